// lt_refine.h -- records and the FP64 expressions shared by the host side (lt_refine.cpp) and the device side
// (lt_kernels_refine.hip) of the geometric line refinement: step [E] of limap.runners.line_triangulation
// (runners/line_triangulation.py:208-219) with constant cameras, where every track is its own 4-degree-of-freedom robust
// least-squares problem.  Both sides compile the same inline functions with -ffp-contract=off, so the
// device and lt_fn_refine_host agree bit for bit.
//
// limap's own part is restated in its operation order where the order decides a branch (the conversions), and as one
// 3x6 matrix per support where it is linear in the Pluecker line (the projection): paths relative to src/limap,
//   base/infinite_line.cc:67-71,180-231,265-287   InfiniteLine3d(Line3d), MinimalInfiniteLine3d, GetInfiniteLine,
//                                                 GetLineSegmentFromInfiniteLine3d
//   base/pose.cc:7-28                             RotationMatrixToQuaternion / QuaternionToRotationMatrix
//   base/linetrack.cc:315-322                     ComputeLineWeights
//   ceresbase/line_transforms.h:8-29              MinimalPluckerToPlucker
//   ceresbase/line_projection.h:14-80             Line_ImgFromCam, Line_WorldToPixel
//   ceresbase/line_dists.h:19-28                  CeresComputeDist2D_cosine
//   optimize/line_refinement/cost_functions.h:96-127  Ceres_PerpendicularDist2D, Ceres_CosineWeightedPerpendicularDist2D_1D
// and the two optional terms of limap.optimize.line_refinement (runners/refinement.py), one block per support each:
//   optimize/line_refinement/cost_functions.h:35-90, refine.cc:87-126   VPConstraintsFunctor, AddVPResiduals
//   ceresbase/line_dists.h:40-57, ceresbase/line_projection.h:125-134   CeresComputeDist3D_sine, GetDirectionFromVP
//   optimize/line_refinement/pixel_cost_functions.h:34-107, refine.cc:315-360   MaxHeatmapFunctor, AddHeatmapResiduals
//   base/linetrack.cc:324-351, base/infinite_line.cc:9-16               ComputeHeatmapSamples, InfiniteLine2d(p, direc)
//   ceresbase/line_transforms.h:55-72                                   Ceres_IntersectLineCoordinates
//   ceresbase/interpolation.h:526-579, features/featuremap.h:71-85      BiLinearInterpolator over a Grid2D, one node
// ASSUMPTIONS of the same kind as lt_svd.h (the libraries are not part of limap; their published procedures are
// followed): Eigen's Quaternion(Matrix3) and Quaternion::toRotationMatrix, Ceres' QuaternionToRotation
// (QuaternionToScaledRotation, then the division by the squared norm), CauchyLoss, ScaledLoss and the Jet rule
// d|x|/dx = +1 at x = 0; for the two terms Ceres' QuaternionRotatePoint (the scale 1 / |q|, then
// UnitQuaternionRotatePoint in its cross-product form, rotation.h of Ceres 2.1 and later), CrossProduct, TrivialLoss,
// HuberLoss (rho' = max(DBL_MIN, a / sqrt s) outside a^2), Grid2D::GetValue (rows and columns clamped to the image), the
// Jet of an interpolated value (dfdr dr + dfdc dc), and Eigen's normalized() of a 2- and a 3-vector taken as
// v / sqrt((x^2 + y^2) + z^2).  `const int row = std::floor(r)` overflows the int for |r| >= 2^31 upstream; here the
// floor stays a double and is clamped to [-3, h] before the conversion, which reads the same texels wherever upstream's
// conversion is defined.  The minimiser is this project's own definition, not Ceres' iterates.
#pragma once

#include "lt_lm.h"

namespace lt {

constexpr int kRfWidth = 16;            // lanes of a wave64 that work on one track (k_refine_lm, k_refine_cut)
constexpr int kRfBlock = 64;            // lanes per workgroup: one wave, four tracks
constexpr int kRfFields = 23;           // doubles per support (SoA over the scene's supports): A[18], x1 y1 x2 y2, weight
constexpr double kRfCauchyB = 0.0625;   // CauchyLoss(0.25): b = a^2 (refinement_config.h:21)
constexpr int kRfTermWidth = 16;        // lanes per track of k_refine_lm_terms and of its host twin (the choice: DESIGN §19)
constexpr int kRfExtFields = 8;         // doubles per support of the terms' table: unit qvec[4], VP direction[3], VP flag
constexpr double kRfHuberA = 0.001;     // HuberLoss(0.001) (refinement_config.h:23)

// the termination codes of a track (lt_refine_get) are RfCode (lt_lm.h)

// a track as the kernels see it: supports [s0, s0 + n) of the scene's supports (residual order), line, flags
struct RfTrack {
  long long s0;
  int n, constant;
};
static_assert(sizeof(RfTrack) == 16, "RfTrack layout");

// per track result
struct RfOut {
  double p[6];      // uvec (w, x, y, z), wvec
  double seg[6];    // start, end
  double cost0, cost1;
  int iters, code;
};
static_assert(sizeof(RfOut) == 120, "RfOut layout");

// ---- exp on [0, 700] and log on [1, inf): plain FP64 arithmetic in a fixed order, the same bits on both sides ----
// exp(x) = 2^k exp(r), k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo, |r| <= 0.3466; exp(r) by its Taylor
// polynomial of degree 14 (Horner); 2^k by ten exact multiplications
LT_HD double lt_exp(double x) {
  const double kd = floor(x * 1.4426950408889634074 + 0.5);
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
  double p = 1.0 / 87178291200.0;
  p = p * r + 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  int k = (int)kd;
  double s = 1.0, b = 2.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    s = (k & 1) ? s * b : s;
    b = b * b;
    k >>= 1;
  }
  return p * s;
}

// log(y), y >= 1 finite: y = 2^e f with f in [1/sqrt 2, sqrt 2) by ten exact scalings, log f = 2 atanh(s),
// s = (f - 1) / (f + 1), |s| <= 0.1716, odd series to s^23
LT_HD double lt_log(double y) {
  int e = 0;
  if (y >= 0x1p512) { y = y * 0x1p-512; e += 512; }
  if (y >= 0x1p256) { y = y * 0x1p-256; e += 256; }
  if (y >= 0x1p128) { y = y * 0x1p-128; e += 128; }
  if (y >= 0x1p64) { y = y * 0x1p-64; e += 64; }
  if (y >= 0x1p32) { y = y * 0x1p-32; e += 32; }
  if (y >= 0x1p16) { y = y * 0x1p-16; e += 16; }
  if (y >= 0x1p8) { y = y * 0x1p-8; e += 8; }
  if (y >= 0x1p4) { y = y * 0x1p-4; e += 4; }
  if (y >= 0x1p2) { y = y * 0x1p-2; e += 2; }
  if (y >= 0x1p1) { y = y * 0x1p-1; e += 1; }
  if (y > 1.41421356237309514547) { y = y * 0.5; e += 1; }
  const double s = (y - 1.0) / (y + 1.0), z = s * s;
  double p = 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z;                       // the series without its leading 1
  const double lf = 2.0 * s + 2.0 * s * p;
  const double ed = (double)e;
  return ed * 6.93147180369123816490e-01 + (lf + ed * 1.90821492927058770002e-10);
}

// the forward-mode scalar (lt_lm.h) along the four local directions (du1, du2, du3, dw)
typedef Jet<4> Rf4;

// MinimalPluckerToPlucker (line_transforms.h:8-29): dm = (d, m) from uvec (w, x, y, z) and wvec
template <class T>
LT_HD void rf_plucker(const T u[4], const T w[2], T dm[6]) {
  const T a = u[0], b = u[1], c = u[2], d = u[3];
  const T aa = a * a, ab = a * b, ac = a * c, ad = a * d, bb = b * b, bc = b * c, bd = b * d, cc = c * c, cd = c * d,
          dd = d * d;
  const T n = ((aa + bb) + cc) + dd;
  const T r0 = (((aa + bb) - cc) - dd) / n, r1 = ((bc - ad) * 2.0) / n;
  const T r3 = ((ad + bc) * 2.0) / n, r4 = (((aa - bb) + cc) - dd) / n;
  const T r6 = ((bd - ac) * 2.0) / n, r7 = ((ab + cd) * 2.0) / n;
  const T w1 = rf_abs(w[0]), w2 = rf_abs(w[1]);
  const T bn = w2 / (w1 + kEps);
  dm[0] = r0; dm[1] = r3; dm[2] = r6;
  dm[3] = r1 * bn; dm[4] = r4 * bn; dm[5] = r7 * bn;
}

// the 3x6 matrix of a view: Line_WorldToPixel (line_projection.h:51-80) before its normalisation is
// A (d, m) with A = cof(K) [ [t]x R | R ] -- R [m]x R^T - t (R d)^T + (R d) t^T = [R m + t x R d]x and
// K [v]x K^T = [cof(K) v]x.  q: CameraPose's quaternion, normalised once like its constructor (camera.h:94-95), then
// Ceres' QuaternionToRotation
// A[f] goes to out[f * stride] (the SoA table directly: no private array of the lane)
LT_HD void rf_view_matrix(const double *k4, const double *q4, const double *t3, double *out, long long stride) {
  // lm_normalise_q's expressions, written out: through the call k_refine_prep needs 70 registers for 62 and loses a wave
  double q[4];
  const double n0 = sqrt((q4[0] * q4[0] + q4[2] * q4[2]) + (q4[1] * q4[1] + q4[3] * q4[3]));
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = n0 > 0.0 ? q4[i] / n0 : q4[i];
  const double a = q[0], b = q[1], c = q[2], d = q[3];
  const double aa = a * a, ab = a * b, ac = a * c, ad = a * d, bb = b * b, bc = b * c, bd = b * d, cc = c * c,
               cd = c * d, dd = d * d;
  const double n = ((aa + bb) + cc) + dd;
  double R[9] = {((aa + bb) - cc) - dd, 2.0 * (bc - ad), 2.0 * (ac + bd), 2.0 * (ad + bc), ((aa - bb) + cc) - dd,
                 2.0 * (cd - ab), 2.0 * (bd - ac), 2.0 * (ab + cd), ((aa - bb) - cc) + dd};
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = R[i] / n;
  // B = [ [t]x R | R ]  (3 x 6, row-major)
  double B[18];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double r0 = R[j], r1 = R[3 + j], r2 = R[6 + j];
    B[j] = t3[1] * r2 - t3[2] * r1;
    B[6 + j] = t3[2] * r0 - t3[0] * r2;
    B[12 + j] = t3[0] * r1 - t3[1] * r0;
    B[3 + j] = r0; B[9 + j] = r1; B[15 + j] = r2;
  }
  // cof(K) = [[fy, 0, 0], [0, fx, 0], [-fy cx, -fx cy, fx fy]]
  const double fx = k4[0], fy = k4[1], cx = k4[2], cy = k4[3];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    out[(long long)j * stride] = fy * B[j];
    out[(long long)(6 + j) * stride] = fx * B[6 + j];
    out[(long long)(12 + j) * stride] = ((-(fy * cx)) * B[j] - (fx * cy) * B[6 + j]) + (fx * fy) * B[12 + j];
  }
}

// one support as the residual reads it (strided by `stride` doubles in the scene's SoA table)
struct RfSup {
  double A[18];
  double x1, y1, x2, y2, weight;
};
LT_HD RfSup rf_load(const double *tab, long long stride, long long s) {
  RfSup r;
  for (int i = 0; i < 18; ++i) r.A[i] = tab[(long long)i * stride + s];
  r.x1 = tab[18 * stride + s]; r.y1 = tab[19 * stride + s];
  r.x2 = tab[20 * stride + s]; r.y2 = tab[21 * stride + s];
  r.weight = tab[22 * stride + s];
  return r;
}

// the two residuals of a support (cost_functions.h:106-127 after Line_WorldToPixel); T = double or Rf4
template <class T>
LT_HD void rf_residual(const RfSup &s, const T dm[6], double alpha, T res[2]) {
  T c[3];
  for (int i = 0; i < 3; ++i) {
    const double *a = s.A + 6 * i;
    c[i] = ((((dm[0] * a[0] + dm[1] * a[1]) + dm[2] * a[2]) + dm[3] * a[3]) + dm[4] * a[4]) + dm[5] * a[5];
  }
  const T cn = rf_sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + kEps);  // Line_ImgFromCam :43-47
  const T c0 = c[0] / cn, c1 = c[1] / cn, c2 = c[2] / cn;
  const T dn = rf_sqrt((c0 * c0 + c1 * c1) + kEps);  // direc_norm
  const T e0 = -(c1 / dn), e1 = c0 / dn;             // dir2d
  const double f0 = s.x2 - s.x1, f1 = s.y2 - s.y1;   // direc
  const T n1 = rf_sqrt((e0 * e0 + e1 * e1) + kEps);
  const double n2 = sqrt((f0 * f0 + f1 * f1) + kEps);
  T cosine = rf_abs((e0 * f0 + e1 * f1) / (n1 * n2));
  if (rf_val(cosine) > 1.0) rf_set(cosine, 1.0);
  const T wgt = rf_exp((1.0 - cosine) * alpha);
  res[0] = (((c0 * s.x1 + c1 * s.y1) + c2) / dn) * wgt;
  res[1] = (((c0 * s.x2 + c1 * s.y2) + c2) / dn) * wgt;
}

// rho_k(s) = w b log(1 + s / b): ScaledLoss(CauchyLoss(0.25), w) over the squared norm of a residual block
LT_HD double rf_rho(double weight, double s) { return (weight * kRfCauchyB) * lt_log(1.0 + s / kRfCauchyB); }
LT_HD double rf_rho1(double weight, double s) { return weight / (1.0 + s / kRfCauchyB); }

// the sums of a linearisation, in the order every reduction uses: H upper triangle (00 01 02 03 11 12 13 22 23 33), g
constexpr int kRfSums = 14;
static_assert(kRfSums == lm_sums(4), "the sums of four unknowns");
LT_HD void rf_accumulate(const RfSup &s, const Rf4 dm[6], double alpha, double acc[kRfSums], double *r2 = nullptr) {
  Rf4 r[2];
  rf_residual<Rf4>(s, dm, alpha, r);
  if (r2) { r2[0] = r[0].v; r2[1] = r[1].v; }
  const double sq = r[0].v * r[0].v + r[1].v * r[1].v;
  const double rho1 = rf_rho1(s.weight, sq);
  int o = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j, ++o) acc[o] = acc[o] + rho1 * (r[0].d[i] * r[0].d[j] + r[1].d[i] * r[1].d[j]);
  for (int i = 0; i < 4; ++i) acc[10 + i] = acc[10 + i] + rho1 * (r[0].d[i] * r[0].v + r[1].d[i] * r[1].v);
}
LT_HD double rf_cost_term(const RfSup &s, const double dm[6], double alpha) {
  double r[2];
  rf_residual<double>(s, dm, alpha, r);
  return rf_rho(s.weight, r[0] * r[0] + r[1] * r[1]);
}

// ---- the VP and the heatmap term (limap.optimize.line_refinement with use_vp / use_heatmap) ----
// the heatmap of an image in the packed texel buffer
struct RfHm {
  long long off;  // first texel
  int h, w;
};
static_assert(sizeof(RfHm) == 16, "RfHm layout");
template <class Tx>
struct RfGrid {
  const Tx *tex;
  int h, w;
};
// the terms' parameters as the kernels read them
struct RfTermCfg {
  double vp_multiplier, heatmap_multiplier;
  double heatmap_den;        // n_samples_heatmap / 10.0
  double t0, interval;       // t_j = t0 + interval * j, interval = (max - min) / (n - 1) (linetrack.cc:329-335)
  int n_samples, use_geometric, use_vp, use_heatmap;
};
// what a support carries for the terms besides RfSup (kRfExtFields doubles, SoA like the support table)
struct RfExt {
  double q[4];    // the view's quaternion times Ceres' scale 1 / |q|
  double vp[3];   // the direction of the support's vanishing point, normalised as the sine normalises it
  double has_vp;  // 1.0 where the VPResult labels the support's line
};
LT_HD RfExt rf_load_ext(const double *ext, long long stride, long long s) {
  RfExt e;
  for (int i = 0; i < 4; ++i) e.q[i] = ext[(long long)i * stride + s];
  for (int i = 0; i < 3; ++i) e.vp[i] = ext[(long long)(4 + i) * stride + s];
  e.has_vp = ext[7 * stride + s];
  return e;
}

// the constants of a support's VP block: CameraPose's normalisation (camera.h:94-95) and the scale of Ceres'
// QuaternionRotatePoint; GetDirectionFromVP (line_projection.h:125-134) and the normalisation CeresComputeDist3D_sine
// applies to its second argument (line_dists.h:42-50).  F[f] goes to out[f * stride]
LT_HD void rf_ext_prep(const double *k4, const double *q4, bool has_vp, const double *vp3, double *out, long long stride) {
  double q[4];
  lm_normalise_q(q4, q);
  const double scale = 1.0 / sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) out[(long long)i * stride] = q[i] * scale;
  double d[3] = {0.0, 0.0, 0.0};
  if (has_vp) {
    d[0] = vp3[0] / k4[0] - (k4[2] / k4[0]) * vp3[2];
    d[1] = vp3[1] / k4[1] - (k4[3] / k4[1]) * vp3[2];
    d[2] = vp3[2];
    const double n = sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + kEps);
    for (int i = 0; i < 3; ++i) d[i] = d[i] / n;
    const double n2 = sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + kEps);
    for (int i = 0; i < 3; ++i) d[i] = d[i] / n2;
  }
  for (int i = 0; i < 3; ++i) out[(long long)(4 + i) * stride] = d[i];
  out[7 * stride] = has_vp ? 1.0 : 0.0;
}

// the residual of a VP block (cost_functions.h:71-84): the sine between the line's direction in the camera frame and
// the VP's direction
template <class T>
LT_HD T rf_vp_residual(const RfExt &e, const T dm[6]) {
  const double *q = e.q;
  T uv0 = dm[2] * q[2] - dm[1] * q[3];  // UnitQuaternionRotatePoint: uv = q.xyz x pt, doubled
  T uv1 = dm[0] * q[3] - dm[2] * q[1];
  T uv2 = dm[1] * q[1] - dm[0] * q[2];
  uv0 = uv0 + uv0; uv1 = uv1 + uv1; uv2 = uv2 + uv2;
  T r0 = dm[0] + uv0 * q[0], r1 = dm[1] + uv1 * q[0], r2 = dm[2] + uv2 * q[0];
  r0 = r0 + (uv2 * q[2] - uv1 * q[3]);
  r1 = r1 + (uv0 * q[3] - uv2 * q[1]);
  r2 = r2 + (uv1 * q[1] - uv0 * q[2]);
  const T n1 = rf_sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + kEps);
  const T a0 = r0 / n1, a1 = r1 / n1, a2 = r2 / n1;
  const T c0 = a1 * e.vp[2] - a2 * e.vp[1], c1 = a2 * e.vp[0] - a0 * e.vp[2], c2 = a0 * e.vp[1] - a1 * e.vp[0];
  T sine = rf_sqrt(((c0 * c0 + c1 * c1) + c2 * c2) + kEps);
  if (rf_val(sine) > 1.0) rf_set(sine, 1.0);
  return sine;
}

// Line_WorldToPixel with the normalisation of Line_ImgFromCam (line_projection.h:43-47): the expressions rf_residual
// starts with
template <class T>
LT_HD void rf_project(const RfSup &s, const T dm[6], T c[3]) {
  for (int i = 0; i < 3; ++i) {
    const double *a = s.A + 6 * i;
    c[i] = ((((dm[0] * a[0] + dm[1] * a[1]) + dm[2] * a[2]) + dm[3] * a[3]) + dm[4] * a[4]) + dm[5] * a[5];
  }
  const T cn = rf_sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + kEps);
  c[0] = c[0] / cn; c[1] = c[1] / cn; c[2] = c[2] / cn;
}

// sample line j of a support (ComputeHeatmapSamples, linetrack.cc:338-349): InfiniteLine2d(start + t (end - start),
// perp_direction()); the caller has checked that the support's length is positive
LT_HD void rf_sample_line(const RfSup &s, double t, double coor[3]) {
  const double ex = s.x2 - s.x1, ey = s.y2 - s.y1;
  const double n = sqrt(ex * ex + ey * ey);
  const double d0 = ex / n, d1 = ey / n;  // direction()
  const double p0 = d1, p1 = -d0;         // perp_direction()
  const double px = s.x1 + t * ex, py = s.y1 + t * ey;
  const double c0 = p1, c1 = -p0, c2 = (-p1) * px + p0 * py;
  const double cn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  coor[0] = c0 / cn; coor[1] = c1 / cn; coor[2] = c2 / cn;
}

// texels widen exactly: binary16 from its bits (no half type on the host side), binary32 by the conversion
LT_HD double rf_widen(unsigned short h) {
  const unsigned long long sign = (unsigned long long)(h >> 15) << 63;
  const int e = (h >> 10) & 31, m = h & 1023;
  if (e == 0) {  // zero and subnormals: m 2^-24
    const double v = (double)m * 0x1p-24;
    return sign ? -v : v;
  }
  const unsigned long long ex = (unsigned long long)(e == 31 ? 2047 : e - 15 + 1023);
  const unsigned long long bits = sign | (ex << 52) | ((unsigned long long)m << 42);
  union { unsigned long long u; double d; } cv;
  cv.u = bits;
  return cv.d;
}
LT_HD double rf_widen(float f) { return (double)f; }
// Grid2D::GetValue: rows and columns clamped to the image
template <class Tx>
LT_HD double rf_texel(const RfGrid<Tx> &g, int r, int c) {
  r = r < 0 ? 0 : (r > g.h - 1 ? g.h - 1 : r);
  c = c < 0 ? 0 : (c > g.w - 1 ? g.w - 1 : c);
  return rf_widen(g.tex[(long long)r * g.w + c]);
}
LT_HD double rf_bilinear(double dx, double dy, double ll, double lr, double ul, double ur) {
  const double v0 = (1.0 - dx) * ll + dx * lr, v1 = (1.0 - dx) * ul + dx * ur;
  return (1.0 - dy) * v0 + dy * v1;
}
// floor(r) and floor(c) as indices; a floor outside [-3, size] reads the texels of that bound (the clamp of rf_texel)
LT_HD void rf_cell(double r, double c, int h, int w, int *row, int *col, double *dy, double *dx) {
  const double fr = floor(r), fc = floor(c);
  *dy = r - fr;
  *dx = c - fc;
  *row = (int)(!(fr >= -3.0) ? -3.0 : (fr > (double)h ? (double)h : fr));  // (a NaN, which no caller passes, reads row 0)
  *col = (int)(!(fc >= -3.0) ? -3.0 : (fc > (double)w ? (double)w : fc));
}
// BiLinearInterpolator::Evaluate (interpolation.h:531-564) at (r, c): the value from 4 texels; as a Jet the value and
// upstream's forward differences, 8 texels, all loaded before the first use
template <class Tx>
LT_HD double rf_interp(const RfGrid<Tx> &g, double r, double c) {
  int row, col;
  double dy, dx;
  rf_cell(r, c, g.h, g.w, &row, &col, &dy, &dx);
  const double ll = rf_texel(g, row, col), lr = rf_texel(g, row, col + 1);
  const double ul = rf_texel(g, row + 1, col), ur = rf_texel(g, row + 1, col + 1);
  return rf_bilinear(dx, dy, ll, lr, ul, ur);
}
template <class Tx>
LT_HD Rf4 rf_interp(const RfGrid<Tx> &g, const Rf4 &r, const Rf4 &c) {
  int row, col;
  double dy, dx;
  rf_cell(r.v, c.v, g.h, g.w, &row, &col, &dy, &dx);
  const double ll = rf_texel(g, row, col), lr = rf_texel(g, row, col + 1);
  const double ul = rf_texel(g, row + 1, col), ur = rf_texel(g, row + 1, col + 1);
  const double lrx = rf_texel(g, row, col + 2), urx = rf_texel(g, row + 1, col + 2);
  const double uly = rf_texel(g, row + 2, col), ury = rf_texel(g, row + 2, col + 1);
  const double f = rf_bilinear(dx, dy, ll, lr, ul, ur);
  const double dfdr = rf_bilinear(dx, dy, ul, ur, uly, ury) - f;
  const double dfdc = rf_bilinear(dx, dy, lr, lrx, ur, urx) - f;
  Rf4 o;
  o.v = f;
  for (int i = 0; i < 4; ++i) o.d[i] = dfdr * r.d[i] + dfdc * c.d[i];
  return o;
}

// one residual of a heatmap block (pixel_cost_functions.h:93-103): 1 - f at the intersection of the projected line c
// with the sample line k (Ceres_IntersectLineCoordinates).  false: the evaluation fails -- |p_homo[2]| < EPS, or not a
// number (a projection that coincides with the sample line), where upstream reads an unset xy
template <class T, class Tx>
LT_HD bool rf_heat_residual(const T c[3], const double k[3], const RfGrid<Tx> &g, T *res) {
  T p0 = c[1] * k[2] - c[2] * k[1], p1 = c[2] * k[0] - c[0] * k[2], p2 = c[0] * k[1] - c[1] * k[0];
  const T n = rf_sqrt((p0 * p0 + p1 * p1) + p2 * p2);
  p0 = p0 / n; p1 = p1 / n; p2 = p2 / n;
  if (!(rf_abs(rf_val(p2)) >= kEps)) {
    rf_set(*res, 0.0);
    return false;
  }
  const T x = p0 / p2, y = p1 / p2;
  *res = 1.0 - rf_interp(g, y, x);
  return true;
}

// ScaledLoss(HuberLoss(a), w) over s, the squared norm of a block, and its derivative
LT_HD double rf_huber(double weight, double s) {
  const double b = kRfHuberA * kRfHuberA;
  return s > b ? weight * ((2.0 * kRfHuberA) * sqrt(s) - b) : weight * s;
}
LT_HD double rf_huber1(double weight, double s) {
  const double b = kRfHuberA * kRfHuberA;
  if (!(s > b)) return weight;
  const double m = kRfHuberA / sqrt(s);
  return weight * (m > 2.2250738585072014e-308 ? m : 2.2250738585072014e-308);
}
// the weights of a support's VP and heatmap blocks (refine.cc:104, 338-339)
LT_HD double rf_vp_weight(const RfSup &s, const RfTermCfg &tc) { return s.weight * tc.vp_multiplier; }
LT_HD double rf_heat_weight(const RfSup &s, const RfTermCfg &tc) { return (s.weight * tc.heatmap_multiplier) / tc.heatmap_den; }

// the cost of a support: geometric + VP + heatmap, in that order; a heatmap block sums its samples in ascending order
// before the loss.  +inf where a sample fails
template <bool HM, class Tx>
LT_HD double rf_cost_terms(const RfSup &s, const RfExt &e, const RfGrid<Tx> &g, const RfTermCfg &tc, const double dm[6],
                           double alpha) {
  double cost = 0.0;
  if (tc.use_geometric) cost = cost + rf_cost_term(s, dm, alpha);
  if (tc.use_vp && e.has_vp != 0.0) {
    const double r = rf_vp_residual<double>(e, dm);
    cost = cost + rf_vp_weight(s, tc) * (r * r);
  }
  if (HM) {
    double c[3], sq = 0.0;
    rf_project<double>(s, dm, c);
    bool ok = true;
    for (int j = 0; j < tc.n_samples; ++j) {
      double k[3], r;
      rf_sample_line(s, tc.t0 + tc.interval * (double)j, k);
      ok = rf_heat_residual<double, Tx>(c, k, g, &r) && ok;
      sq = sq + r * r;
    }
    cost = ok ? cost + rf_huber(rf_heat_weight(s, tc), sq) : __builtin_inf();
  }
  return cost;
}

// rf_accumulate with the terms: the blocks of a support add to acc in the order geometric, VP, heatmap; a heatmap block
// first sums its samples' products in ascending order, then applies the loss' derivative.  res (host, tests): the
// residuals of the support, 2 geometric, 1 VP, n_samples heatmap, NaN where a block is absent.  false where a heatmap
// sample fails (its sample adds nothing)
template <bool HM, class Tx>
LT_HD bool rf_accumulate_terms(const RfSup &s, const RfExt &e, const RfGrid<Tx> &g, const RfTermCfg &tc, const Rf4 dm[6],
                               double alpha, double acc[kRfSums], double *res = nullptr) {
  if (tc.use_geometric) rf_accumulate(s, dm, alpha, acc, res);
  if (tc.use_vp && e.has_vp != 0.0) {
    const Rf4 r = rf_vp_residual<Rf4>(e, dm);
    const double rho1 = rf_vp_weight(s, tc);
    if (res) res[2] = r.v;
    int o = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j, ++o) acc[o] = acc[o] + rho1 * (r.d[i] * r.d[j]);
    for (int i = 0; i < 4; ++i) acc[10 + i] = acc[10 + i] + rho1 * (r.d[i] * r.v);
  }
  bool ok = true;
  if (HM) {
    Rf4 c[3];
    rf_project<Rf4>(s, dm, c);
    double blk[kRfSums], sq = 0.0;
    for (int o = 0; o < kRfSums; ++o) blk[o] = 0.0;
    for (int n = 0; n < tc.n_samples; ++n) {
      double k[3];
      Rf4 r;
      rf_sample_line(s, tc.t0 + tc.interval * (double)n, k);
      ok = rf_heat_residual<Rf4, Tx>(c, k, g, &r) && ok;
      if (res) res[3 + n] = r.v;
      sq = sq + r.v * r.v;
      int o = 0;
      for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j, ++o) blk[o] = blk[o] + r.d[i] * r.d[j];
      for (int i = 0; i < 4; ++i) blk[10 + i] = blk[10 + i] + r.d[i] * r.v;
    }
    const double rho1 = rf_huber1(rf_heat_weight(s, tc), sq);
    for (int o = 0; o < kRfSums; ++o) acc[o] = acc[o] + rho1 * blk[o];
  }
  return ok;
}

// the point and its four local directions: u + du_i (0, e_i) (x) u, w + dw (-w1, w0)
LT_HD void rf_seed(const double p[6], Rf4 u[4], Rf4 w[2]) {
  lm_seed_quat(p, u);
  w[0] = Rf4(p[4]); w[0].d[3] = -p[5];
  w[1] = Rf4(p[5]); w[1].d[3] = p[4];
}

// the chart of a line: u+ = normalize((1, du) (x) u), w+ = normalize(w + dw (-w1, w0))
struct RfChart {
  static constexpr int kParams = 6, kStep = 4;
  static LT_HD void retract(const double p[6], const double dl[4], double out[6]) {
    lm_retract_quat(p, dl, out);
    const double w0 = p[4] - dl[3] * p[5], w1 = p[5] + dl[3] * p[4];
    const double nw = sqrt(w0 * w0 + w1 * w1);
    out[4] = w0 / nw; out[5] = w1 / nw;
  }
};

// the minimiser of one track: lm_loop over the line's chart.  G supplies the two reductions over the
// track's supports, cost(p) and linearise(p, acc).  rf_lm_from: after the first cost evaluation F (the cost at p); a
// constant track keeps its parameters.  rf_lm has no finiteness check of its own
template <class G>
LT_HD void rf_lm_from(G &grp, double F, bool constant, int max_iter, double p[6], double *cost1, int *iters, int *code_out) {
  if (constant) lm_skip(F, kRfConstant, cost1, iters, code_out);
  else lm_loop<RfChart>(grp, F, max_iter, p, cost1, iters, code_out);
}
template <class G>
LT_HD void rf_lm(G &grp, bool constant, int max_iter, double p[6], double *cost0, double *cost1, int *iters, int *code_out) {
  const double F = grp.cost(p);
  *cost0 = F;
  rf_lm_from(grp, F, constant, max_iter, p, cost1, iters, code_out);
}

// rf_lm with the VP and heatmap terms: a cost evaluation in which a sample fails is +inf (non-finite texels make it
// +inf or NaN), so the ratio test rejects the step and the radius shrinks; at the initial point the track ends with
// kRfEvalFailed, its parameters unchanged, as Ceres' FAILURE leaves the line (a constant track reports kRfConstant first)
template <class G>
LT_HD void rf_lm_terms(G &grp, bool constant, int max_iter, double p[6], double *cost0, double *cost1, int *iters,
                       int *code_out) {
  const double F = grp.cost(p);
  *cost0 = F;
  if (!(F <= kMaxDist)) lm_skip(F, constant ? kRfConstant : kRfEvalFailed, cost1, iters, code_out);
  else rf_lm_from(grp, F, constant, max_iter, p, cost1, iters, code_out);
}

LT_HD void rf_quat_from_matrix(const double m[3][3], double p[4]);

// MinimalInfiniteLine3d(InfiniteLine3d(line)) (infinite_line.cc:67-71,180-223); the caller has checked length > 0
LT_HD void rf_minimal(const double l6[6], double p[6]) {
  const d3 s = mk3(l6[0], l6[1], l6[2]);
  const d3 a = unit(sub(mk3(l6[3], l6[4], l6[5]), s));  // Line3d::direction()
  const d3 b = cross(s, a);
  const double bn = sqrt(sqn(b));
  const double den = sqrt(1.0 * 1.0 + bn * bn);
  p[4] = 1.0 / den;
  p[5] = bn / den;
  const double an = sqrt(sqn(a));
  const d3 c0 = mk3(a.x / an, a.y / an, a.z / an);
  d3 c1, c2;
  if (bn > kEps) {
    c1 = mk3(b.x / bn, b.y / bn, b.z / bn);
    const d3 axb = cross(a, b);
    const double n = sqrt(sqn(axb));
    c2 = mk3(axb.x / n, axb.y / n, axb.z / n);
  } else {
    const double av[3] = {a.x, a.y, a.z};
    int best = 0;
    if (fabs(av[1]) > fabs(av[0])) best = 1;
    if (fabs(av[2]) > fabs(av[best])) best = 2;
    const int i1 = (best + 1) % 3, i2 = (best + 2) % 3;
    double bp[3];
    bp[i1] = 1.0;
    bp[i2] = 1.0;
    bp[best] = -(av[i1] * bp[i1] + av[i2] * bp[i2]) / av[best];
    const d3 bv = mk3(bp[0], bp[1], bp[2]);
    const double n1 = sqrt(sqn(bv));
    c1 = mk3(bv.x / n1, bv.y / n1, bv.z / n1);
    const d3 axb = cross(a, bv);
    const double n = sqrt(sqn(axb));
    c2 = mk3(axb.x / n, axb.y / n, axb.z / n);
  }
  // Eigen::Quaterniond(Q), Q = [c0 c1 c2] by columns: m(i, j) = column j, row i
  const double m[3][3] = {{c0.x, c1.x, c2.x}, {c0.y, c1.y, c2.y}, {c0.z, c1.z, c2.z}};
  rf_quat_from_matrix(m, p);
}

// Eigen's Quaternion(Matrix3): (w, x, y, z) of the rotation matrix m (row, column)
LT_HD void rf_quat_from_matrix(const double m[3][3], double p[4]) {
  double t = (m[0][0] + m[1][1]) + m[2][2];
  double q[4];  // x, y, z, w
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
  }
  p[0] = q[3]; p[1] = q[0]; p[2] = q[1]; p[3] = q[2];
}

// GetInfiniteLine() (infinite_line.cc:225-231): d, m from the minimal parameters
LT_HD void rf_infinite(const double p[6], d3 *d, d3 *m) {
  const double n = sqrt((p[0] * p[0] + p[2] * p[2]) + (p[1] * p[1] + p[3] * p[3]));  // NormalizeQuaternion (pose.cc:19-28)
  double w, x, y, z;
  if (n == 0.0) {
    w = 1.0; x = p[1]; y = p[2]; z = p[3];
  } else {
    w = p[0] / n; x = p[1] / n; y = p[2] / n; z = p[3] / n;
  }
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  *d = mk3(1.0 - (tyy + tzz), txy + twz, txz - twy);  // Q.col(0)
  const double f = fabs(p[5]) / fabs(p[4]);
  *m = mk3(f * (txy - twz), f * (1.0 - (txx + tzz)), f * (tyz + twx));  // f * Q.col(1)
}

// GetLineSegmentFromInfiniteLine3d (infinite_line.cc:265-287), the projection of its values: value 2 k + e of a
// track is (endpoint e of line3d k - p_ref) . dir
LT_HD d3 rf_pref(d3 d, d3 m, d3 q) {  // point_projection (:73-78)
  const d3 mq = add(m, cross(d, q));
  return add(q, cross(d, mq));
}
LT_HD double rf_value(const double *l3d6, long long j, d3 pref, d3 dir) {
  const double *e = l3d6 + 3 * j;  // 6 doubles per line: value j reads point j of the flat list
  return dot(sub(mk3(e[0], e[1], e[2]), pref), dir);
}

// does value i hold rank r of the n values?  #(< v_i) <= r < #(< v_i) + #(== v_i), and i is the first index with its
// value (-0.0 == +0.0: the lowest index speaks for both, so one lane writes and the host picks the same element).  A NaN
// among the values satisfies no rank; the caller then returns NaN
LT_HD void rf_rank_test(const double *l3d6, long long n, long long i, d3 pref, d3 dir, long long lo, long long hi,
                        double *v_out, bool *is_lo, bool *is_hi) {
  const double v = rf_value(l3d6, i, pref, dir);
  long long lt = 0, eq = 0;
  bool first = true;
  for (long long j = 0; j < n; ++j) {
    const double o = rf_value(l3d6, j, pref, dir);
    lt += o < v;
    eq += o == v;
    if (j < i && o == v) first = false;
  }
  *v_out = v;
  *is_lo = first && lt <= lo && lo < lt + eq;
  *is_hi = first && lt <= hi && hi < lt + eq;
}

static_assert(kRfBlock % kRfTermWidth == 0 && (kRfTermWidth & (kRfTermWidth - 1)) == 0, "a group is a power-of-two part of a wave");

// the scene's tables on the device
struct RfDev {
  const RfTrack *tracks;
  long long n_tracks;
  const double *sup;        // kRfFields x stride
  long long stride;
  const double *l3d;        // 6 doubles per support, member order
  double alpha;
  int max_iter, num_outliers;
};

// the terms' tables on the device: the supports' extra fields and heatmap slots, the heatmap table and the texels the
// context holds (RefineState)
struct RfDevTerms {
  const double *ext;     // kRfExtFields x stride
  const int *sup_hm;     // per support its row of hm (heatmap term only)
  const RfHm *hm;
  const void *texels;    // unsigned short (binary16) or float
  RfTermCfg cfg;
};

// ---- the groups of rf_lm and rf_lm_terms over the lanes (LmWaveLanes in the kernels, LmHostLanes in the host twins) ----
// the supports of a track, lane l taking supports l, l + kRfWidth, ...
template <class Lanes>
struct RfGroup {
  Lanes lanes;
  const double *sup;  // kRfFields x stride
  long long stride;
  const RfTrack &t;
  double alpha;
  LT_HD double cost(const double p[6]) const {
    double dm[6], s;
    rf_plucker<double>(p, p + 4, dm);
    lanes.template over<1>(t.n, 1, [&](int k, double *a) { a[0] = a[0] + rf_cost_term(rf_load(sup, stride, t.s0 + k), dm, alpha); }, &s);
    return 0.5 * s;
  }
  LT_HD void linearise(const double p[6], double acc[kRfSums]) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    lanes.template over<kRfSums>(t.n, kRfSums, [&](int k, double *a) { rf_accumulate(rf_load(sup, stride, t.s0 + k), dm, alpha, a); }, acc);
  }
};

// RfGroup with the terms' blocks.  The supports go to the first kRfTermWidth lanes, however many the group has: the
// lanes past them add zeros to the tree, so the wave of k_refine_lm_feat gets k_refine_lm_terms' bits for them.
// Grids: where a support's heatmap comes from, grid<Tx>(s).  The host twins of k_refine_lm_terms and k_refine_lm_feat
// are this group; the two kernels keep device groups of their own
template <class Lanes, bool HM, class Tx, class Grids>
struct RfGroupTerms {
  Lanes lanes;
  const double *sup, *ext;  // kRfFields, kRfExtFields x stride
  long long stride;
  const RfTrack &t;
  double alpha;
  const RfTermCfg &cfg;
  const Grids &grids;
  LT_HD RfGrid<Tx> grid(long long s) const { return HM ? grids.template grid<Tx>(s) : RfGrid<Tx>{nullptr, 1, 1}; }
  // the sum of the supports' costs, and of their blocks at dm (res: the residuals of every support, 3 + n_samples
  // each; false where a heatmap sample of the lane's supports fails: tests, on the host)
  LT_HD double cost_sum(const double p[6]) const {
    double dm[6], total;
    rf_plucker<double>(p, p + 4, dm);
    lanes.template over<1, kRfTermWidth>(t.n, 1, [&](int k, double *a) {
      const long long s = t.s0 + k;
      a[0] = a[0] + rf_cost_terms<HM, Tx>(rf_load(sup, stride, s), rf_load_ext(ext, stride, s), grid(s), cfg, dm, alpha);
    }, &total);
    return total;
  }
  LT_HD bool lin_sums(const Rf4 dm[6], double acc[kRfSums], double *res) const {
    bool ok = true;
    lanes.template over<kRfSums, kRfTermWidth>(t.n, kRfSums, [&](int k, double *a) {
      const long long s = t.s0 + k;
      ok = rf_accumulate_terms<HM, Tx>(rf_load(sup, stride, s), rf_load_ext(ext, stride, s), grid(s), cfg, dm, alpha, a,
                                       res ? res + (size_t)k * (3 + (size_t)cfg.n_samples) : nullptr) && ok;
    }, acc);
    return ok;
  }
  LT_HD double cost(const double p[6]) const { return 0.5 * cost_sum(p); }
  LT_HD bool linearise_res(const double p[6], double acc[kRfSums], double *res) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    return lin_sums(dm, acc, res);
  }
  LT_HD void linearise(const double p[6], double acc[kRfSums]) const { linearise_res(p, acc, nullptr); }
};

// ---- the feature-consistency term (limap.optimize.line_refinement with use_feature) ----
// Restated in upstream's operation order down to the association of every sum (DESIGN §26 writes the order out; the
// tests hold the residuals to a NumPy restatement bit for bit): paths relative to src/limap,
//   optimize/line_refinement/pixel_cost_functions.h:198-400, refine.cc:363-543   FeatureConsisTgtFunctor and its blocks
//   ceresbase/line_projection.h:136-213    GetEpipolarLineCoordinate, Ceres_GetIntersection2dFromInfiniteLine3d
//   ceresbase/line_transforms.h:8-29, line_projection.h:14-80   MinimalPluckerToPlucker with Ceres' QuaternionToRotation
//                                          (the product by the reciprocal of the squared norm), Line_WorldToPixel as the
//                                          products R [m]x R^T - t (R d)^T + (R d) t^T and K [m']x K^T, every 3x3
//                                          product summed left to right -- not the 3x6 matrix of rf_view_matrix
//   features/featurepatch.h:53-123, featuremap.h:77-85   GlobalToLocal, Evaluate at (row = local y, col = local x)
//   ceresbase/interpolation.h:526-579      the bilinear rule of rf_interp over 128 interleaved channels
constexpr int kRfChannels = 128;
constexpr int kRfFeatLanes = 64;                            // one wave64 per track; lane l owns channels 2 l and 2 l + 1
constexpr int kRfFeatBlock = 256;                           // lanes per workgroup of k_refine_lm_feat
constexpr int kRfFeatTracks = kRfFeatBlock / kRfFeatLanes;  // tracks per workgroup
constexpr int kRfFeatSums = kRfSums + 1;                    // the sums of a block: kRfSums and the squared norm
constexpr int kRfFeatMaxImages = kRfFeatLanes;              // lane i projects the line into image i of the track
static_assert(kRfChannels == 2 * kRfFeatLanes, "two channels per lane");
static_assert(kRfTermWidth <= kRfFeatLanes, "the supports go to the first kRfTermWidth lanes of the wave");

// a camera as the term reads it: Ceres' rotation of CameraPose's normalised quaternion, row-major
struct RfFView {
  double R[9], t[3], k[4];
};
static_assert(sizeof(RfFView) == 128, "RfFView layout");
// the grid of a (track, sorted image): h x w x 128 texels and local = R (xy - t); a map is the identity
struct RfFImg {
  const void *tex;
  int h, w;
  double R[4], t[2];
  int cam, pad_;   // row of the views
};
static_assert(sizeof(RfFImg) == 72, "RfFImg layout");
// a kept sample with at least one target: the sample line, the weight of its blocks, its targets [tgt0, tgt0 + n_tgt)
struct RfFSample {
  double k[3], weight;
  long long tgt0;
  int ref, n_tgt;  // ref and the targets: images of the track, 0 .. n_img - 1 in ascending id
};
static_assert(sizeof(RfFSample) == 48, "RfFSample layout");
struct RfFTrack {
  long long img0, smp0, pair0;  // first image, first sample, first fundamental matrix (pair0 + ref n_img + tgt)
  int n_img, n_smp;
};
static_assert(sizeof(RfFTrack) == 32, "RfFTrack layout");
// the term's tables on the device
struct RfDevFeat {
  const RfFTrack *ftracks;
  const RfFImg *imgs;
  const RfFView *views;
  const RfFSample *smps;
  const int *tgts;
  const double *pairs;  // 9 doubles each, row-major
};

LT_HD void rf_fview_prep(const double *k4, const double *q4, const double *t3, RfFView *v) {
  double q[4];
  lm_normalise_q(q4, q);
  const double a = q[0], b = q[1], c = q[2], d = q[3];
  const double aa = a * a, ab = a * b, ac = a * c, ad = a * d, bb = b * b, bc = b * c, bd = b * d, cc = c * c,
               cd = c * d, dd = d * d;
  const double R[9] = {((aa + bb) - cc) - dd, 2.0 * (bc - ad), 2.0 * (ac + bd), 2.0 * (ad + bc), ((aa - bb) + cc) - dd,
                       2.0 * (cd - ab), 2.0 * (bd - ac), 2.0 * (ab + cd), ((aa - bb) - cc) + dd};
  const double n = 1.0 / (((aa + bb) + cc) + dd);
  for (int i = 0; i < 9; ++i) v->R[i] = R[i] * n;
  for (int i = 0; i < 3; ++i) v->t[i] = t3[i];
  for (int i = 0; i < 4; ++i) v->k[i] = k4[i];
}

// the fundamental matrix of GetEpipolarLineCoordinate (line_projection.h:150-191), constant per (reference, target):
// relR = R_tgt R_ref^T, relT = t_tgt - relR t_ref, E = [relT]x relR, F = (Kinv_tgt^T E) Kinv_ref; every product sums its
// three terms left to right, zero entries included
LT_HD void rf_fundamental(const RfFView &ref, const RfFView &tgt, double F[9]) {
  double Rrt[9], relR[9];
  tr3(ref.R, Rrt);
  mm(tgt.R, Rrt, relR);
  const d3 rt = mv(relR, mk3(ref.t[0], ref.t[1], ref.t[2]));
  const d3 relT = mk3(tgt.t[0] - rt.x, tgt.t[1] - rt.y, tgt.t[2] - rt.z);
  const double sk[9] = {0.0, -relT.z, relT.y, relT.z, 0.0, -relT.x, -relT.y, relT.x, 0.0};
  double E[9], Kitt[9], tmp[9];
  mm(sk, relR, E);
  const double Kir[9] = {1.0 / ref.k[0], 0.0, -ref.k[2] / ref.k[0], 0.0, 1.0 / ref.k[1], -ref.k[3] / ref.k[1], 0.0, 0.0, 1.0};
  const double Kit[9] = {1.0 / tgt.k[0], 0.0, -tgt.k[2] / tgt.k[0], 0.0, 1.0 / tgt.k[1], -tgt.k[3] / tgt.k[1], 0.0, 0.0, 1.0};
  tr3(Kit, Kitt);
  mm(Kitt, E, tmp);
  mm(tmp, Kir, F);
}

// MinimalPluckerToPlucker with Ceres' QuaternionToRotation as published: the scaled rotation times 1 / |u|^2
template <class T>
LT_HD void rf_plucker_c(const T u[4], const T w[2], T d[3], T m[3]) {
  const T a = u[0], b = u[1], c = u[2], e = u[3];
  const T aa = a * a, ab = a * b, ac = a * c, ae = a * e, bb = b * b, bc = b * c, be = b * e, cc = c * c, ce = c * e,
          ee = e * e;
  const T n = rf_inv(((aa + bb) + cc) + ee);
  const T r0 = (((aa + bb) - cc) - ee) * n, r1 = ((bc - ae) * 2.0) * n;
  const T r3 = ((ae + bc) * 2.0) * n, r4 = (((aa - bb) + cc) - ee) * n;
  const T r6 = ((be - ac) * 2.0) * n, r7 = ((ab + ce) * 2.0) * n;
  const T w1 = rf_abs(w[0]), w2 = rf_abs(w[1]);
  const T bn = w2 / (w1 + kEps);
  d[0] = r0; d[1] = r3; d[2] = r6;
  m[0] = r1 * bn; m[1] = r4 * bn; m[2] = r7 * bn;
}

// Line_WorldToPixel of a constant camera (lm_w2p, lt_lm.h)
template <class T>
LT_HD void rf_w2p(const RfFView &v, const T d[3], const T m[3], T c[3]) {
  lm_w2p<T, double>(v.k, v.R, v.t, d, m, c);
}

// Ceres_IntersectLineCoordinates (line_transforms.h:55-72) of the projected line c with the line k, the rule of
// rf_heat_residual; k is a constant (the sample line) or moves with the line (the epipolar line)
template <class T, class K>
LT_HD bool rf_intersect(const T c[3], const K k[3], T *x, T *y) {
  T p0 = c[1] * k[2] - c[2] * k[1], p1 = c[2] * k[0] - c[0] * k[2], p2 = c[0] * k[1] - c[1] * k[0];
  const T n = rf_sqrt((p0 * p0 + p1 * p1) + p2 * p2);
  p0 = p0 / n; p1 = p1 / n; p2 = p2 / n;
  if (!(rf_abs(rf_val(p2)) >= kEps)) {
    rf_set(*x, 0.0);
    rf_set(*y, 0.0);
    return false;
  }
  *x = p0 / p2;
  *y = p1 / p2;
  return true;
}

// (F (x, y, 1)).normalized(): unchanged where the squared norm is not positive
template <class T>
LT_HD void rf_epiline(const double *F, const T &x, const T &y, T e[3]) {
  for (int i = 0; i < 3; ++i) e[i] = (x * F[3 * i] + y * F[3 * i + 1]) + F[3 * i + 2];
  const T z = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  if (rf_val(z) > 0.0) {
    const T n = rf_sqrt(z);
    e[0] = e[0] / n; e[1] = e[1] / n; e[2] = e[2] / n;
  }
}

// FeaturePatch::GlobalToLocal (featurepatch.h:53-67)
template <class T>
LT_HD void rf_to_local(const RfFImg &g, const T &x, const T &y, T *lx, T *ly) {
  const T ax = x - g.t[0], ay = y - g.t[1];
  *lx = ax * g.R[0] + ay * g.R[1];
  *ly = ax * g.R[2] + ay * g.R[3];
}

// the two channels of a lane at texel (r, c), clamped like Grid2D::GetValue: one 4-byte (binary16) or 8-byte (float) load
LT_HD void rf_texel2(const unsigned short *tex, int h, int w, int r, int c, int lane, double out[2]) {
  r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
  c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
  const unsigned short *p = tex + ((long long)r * w + c) * kRfChannels + 2 * lane;
  unsigned int bits;
  __builtin_memcpy(&bits, __builtin_assume_aligned(p, 4), 4);
  out[0] = rf_widen((unsigned short)(bits & 0xffffu));
  out[1] = rf_widen((unsigned short)(bits >> 16));
}
LT_HD void rf_texel2(const float *tex, int h, int w, int r, int c, int lane, double out[2]) {
  r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
  c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
  const float *p = tex + ((long long)r * w + c) * kRfChannels + 2 * lane;
  float f[2];
  __builtin_memcpy(f, __builtin_assume_aligned(p, 8), 8);
  out[0] = rf_widen(f[0]);
  out[1] = rf_widen(f[1]);
}
// BiLinearInterpolator::Evaluate at (row, col) for the lane's two channels: the value from 4 texels, the Jet from 8
template <class Tx>
LT_HD void rf_feat_value(const RfFImg &g, double r, double c, int lane, double f[2]) {
  int row, col;
  double dy, dx, ll[2], lr[2], ul[2], ur[2];
  const Tx *tex = static_cast<const Tx *>(g.tex);
  rf_cell(r, c, g.h, g.w, &row, &col, &dy, &dx);
  rf_texel2(tex, g.h, g.w, row, col, lane, ll);
  rf_texel2(tex, g.h, g.w, row, col + 1, lane, lr);
  rf_texel2(tex, g.h, g.w, row + 1, col, lane, ul);
  rf_texel2(tex, g.h, g.w, row + 1, col + 1, lane, ur);
  for (int ch = 0; ch < 2; ++ch) f[ch] = rf_bilinear(dx, dy, ll[ch], lr[ch], ul[ch], ur[ch]);
}
template <class Tx>
LT_HD void rf_feat_jet(const RfFImg &g, double r, double c, int lane, double f[2], double dfdr[2], double dfdc[2]) {
  int row, col;
  double dy, dx, ll[2], lr[2], ul[2], ur[2], lrx[2], urx[2], uly[2], ury[2];
  const Tx *tex = static_cast<const Tx *>(g.tex);
  rf_cell(r, c, g.h, g.w, &row, &col, &dy, &dx);
  rf_texel2(tex, g.h, g.w, row, col, lane, ll);
  rf_texel2(tex, g.h, g.w, row, col + 1, lane, lr);
  rf_texel2(tex, g.h, g.w, row + 1, col, lane, ul);
  rf_texel2(tex, g.h, g.w, row + 1, col + 1, lane, ur);
  rf_texel2(tex, g.h, g.w, row, col + 2, lane, lrx);
  rf_texel2(tex, g.h, g.w, row + 1, col + 2, lane, urx);
  rf_texel2(tex, g.h, g.w, row + 2, col, lane, uly);
  rf_texel2(tex, g.h, g.w, row + 2, col + 1, lane, ury);
  for (int ch = 0; ch < 2; ++ch) {
    f[ch] = rf_bilinear(dx, dy, ll[ch], lr[ch], ul[ch], ur[ch]);
    dfdr[ch] = rf_bilinear(dx, dy, ul[ch], ur[ch], uly[ch], ury[ch]) - f[ch];
    dfdc[ch] = rf_bilinear(dx, dy, lr[ch], lrx[ch], ur[ch], urx[ch]) - f[ch];
  }
}

// the wave-uniform geometry of a sample and of a block: local coordinates on the reference and on the target grid.
// false: an intersection fails
template <class T>
LT_HD bool rf_feat_ref_xy(const T c_ref[3], const RfFSample &s, const RfFImg &g, T *x, T *y, T *lx, T *ly) {
  const bool ok = rf_intersect<T, double>(c_ref, s.k, x, y);
  rf_to_local<T>(g, *x, *y, lx, ly);
  return ok;
}
template <class T>
LT_HD bool rf_feat_tgt_xy(const T c_tgt[3], const double *F, const T &x, const T &y, const RfFImg &g, T *lx, T *ly) {
  T e[3], xt, yt;
  rf_epiline<T>(F, x, y, e);
  const bool ok = rf_intersect<T, T>(c_tgt, e, &xt, &yt);
  rf_to_local<T>(g, xt, yt, lx, ly);
  return ok;
}

// a lane's two channels of the reference side of a sample: values and derivatives
struct RfFRef {
  double f[2], d[2][4];
};
template <class Tx>
LT_HD void rf_feat_ref_lane(const RfFImg &g, const Rf4 &lx, const Rf4 &ly, int lane, RfFRef *o) {
  double fr[2], fc[2];
  rf_feat_jet<Tx>(g, ly.v, lx.v, lane, o->f, fr, fc);
  for (int ch = 0; ch < 2; ++ch)
    for (int i = 0; i < 4; ++i) o->d[ch][i] = fr[ch] * ly.d[i] + fc[ch] * lx.d[i];
}
// a lane's part of a block's sums (part starts at zero): channel 2 l, then 2 l + 1; the order of rf_accumulate, then
// the squared norm.  res2 (host, tests): the lane's two residuals
template <class Tx>
LT_HD void rf_feat_block_lane(const RfFImg &g, const Rf4 &lx, const Rf4 &ly, const RfFRef &ref, int lane,
                              double part[kRfFeatSums], double *res2 = nullptr) {
  double f[2], fr[2], fc[2];
  rf_feat_jet<Tx>(g, ly.v, lx.v, lane, f, fr, fc);
  for (int ch = 0; ch < 2; ++ch) {
    const double v = f[ch] - ref.f[ch];
    double d[4];
    for (int i = 0; i < 4; ++i) d[i] = (fr[ch] * ly.d[i] + fc[ch] * lx.d[i]) - ref.d[ch][i];
    if (res2) res2[ch] = v;
    int o = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j, ++o) part[o] = part[o] + d[i] * d[j];
    for (int i = 0; i < 4; ++i) part[10 + i] = part[10 + i] + d[i] * v;
    part[kRfSums] = part[kRfSums] + v * v;
  }
}
// a lane's part of a block's squared norm from the values alone
template <class Tx>
LT_HD double rf_feat_sq_lane(const RfFImg &g, double lx, double ly, const double fref[2], int lane) {
  double f[2];
  rf_feat_value<Tx>(g, ly, lx, lane, f);
  const double v0 = f[0] - fref[0], v1 = f[1] - fref[1];
  return (0.0 + v0 * v0) + v1 * v1;
}

void launch_refine_prep(hipStream_t st, const double *kvec, const double *qvec, const double *tvec, const int *sup_cam,
                        const double *l2d4, long long n_sup, double *sup_tab, long long stride, const double *line6,
                        long long n_tracks, RfOut *out);
void launch_refine_lm(hipStream_t st, const RfDev &dev, RfOut *out);
void launch_refine_cut(hipStream_t st, const RfDev &dev, RfOut *out);
void launch_refine_prep_terms(hipStream_t st, const double *kvec, const double *qvec, const int *sup_cam,
                              const int *vp_flag, const double *vp3, long long n_sup, double *ext, long long stride);
// texel_f32: the texels are float, not binary16; only read with cfg.use_heatmap
void launch_refine_lm_terms(hipStream_t st, const RfDev &dev, const RfDevTerms &terms, bool texel_f32, RfOut *out);
// k_refine_lm_feat: the tracks' feature blocks besides the terms'; texel_f32: the type of the features (and of the
// heatmaps, where cfg.use_heatmap)
void launch_refine_lm_feat(hipStream_t st, const RfDev &dev, const RfDevTerms &terms, const RfDevFeat &feat, bool texel_f32,
                           RfOut *out);

}  // namespace lt
