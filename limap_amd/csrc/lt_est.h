// lt_est.h -- the minimal-solver core of limap_amd.estimators: p3p, p2p1ll, p1p2ll and p3ll as ONE problem,
// shared text of the device (lt_kernels_est.hip) and the host twin (lt_est.cpp).  FP64, compiled with -ffp-contract=off
// on both sides, no math library beyond sqrt: both sides compute the same bits.
//
// A sample is np points (unit bearing x, world point X) and nl = 3 - np lines (unit image-line normal l, a point C and
// the unit direction V of the 3D line), built as JointPoseEstimator::MinimalSolver builds them
// (estimators/absolute_pose/joint_pose_estimator.cc:80-110).  With M(q) = |q|^2 R(q), q = (w, x, y, z), t' = |q|^2 t,
// every constraint is  n^T M(q) Y + sigma n^T t' = 0:
//   point  two rows, sigma = 1: n = u, v spanning the plane orthogonal to x, Y = X
//   line   one row, sigma = 1: n = l, Y = C; one row, sigma = 0: n = l, Y = V
// The m = 2 np + nl rows with sigma = 1 are triangularised by Householder reflections of their normals N (m x 3): the
// rows below the third are free of t' (a basis of the left null space of N), the three on top give t' = -N^+ b(q) by back
// substitution.  Together with the sigma = 0 rows that is always three quadrics q^T A_k q = 0; in the chart w = 1 they
// are solved through the octic in z described in DESIGN §30.  Every guard is an explicit pivot test: a sample that fails
// one returns fewer (or no) poses, never a NaN pose.
#pragma once

#include "lt_geom.h"

namespace lt {

constexpr int kEsP3P = 0, kEsP2P1LL = 1, kEsP1P2LL = 2, kEsP3LL = 3;
constexpr int kEsMaxSol = 8;       // poses of one sample
constexpr int kEsFields = 45;      // x X l C V, 3 x 3 each, of one sample (unused entries 0)
constexpr int kEsPoseDoubles = 7;  // qvec (w x y z), tvec
constexpr int kEsBlock = 64;       // k_est_minimal: one lane per sample
// the definition's constants
constexpr double kEsRankTol = 1e-10;    // Householder column norm of the normals, normals of unit length
constexpr double kEsPivotTol = 1e-10;   // pivots of the constant block, rows scaled to max-abs 1
constexpr double kEsLeadTol = 1e-14;    // leading coefficient of the octic against its largest
constexpr double kEsChainTol = 1e-12;   // a Sturm remainder's coefficients against its dividend (max-abs 1)
constexpr int kEsBisect = 56;           // Sturm bisections per root inside the Cauchy bound
constexpr int kEsRootNewton = 4;        // Newton steps on the octic
constexpr int kEsPolish = 3;            // Newton steps of (x, y, z, t') on the six constraints
constexpr double kEsNewtonTol = 1e-13;  // pivots of the polish against the Jacobian's largest entry
constexpr double kEsResidualTol = 1e-9; // a pose's six normalised constraints (sines of angles)

// the two large functions (es_octic_roots, es_solve): not LT_HD's __forceinline__, so that a caller with several call
// sites does not carry several copies of their arrays
#define ES_HD __host__ __device__ inline

LT_HD double es_abs(double v) { return v < 0.0 ? -v : v; }
LT_HD bool es_finite(double v) { return v - v == 0.0; }

LT_HD int es_num_points(int kind) { return 3 - kind; }

// monomials of q = (w, x, y, z): w2 wx wy wz x2 xy xz y2 yz z2
LT_HD void es_quad_row(const double n[3], const double Y[3], double c[10]) {
  const double d0 = n[0] * Y[0], d1 = n[1] * Y[1], d2 = n[2] * Y[2];
  c[0] = (d0 + d1) + d2;
  c[1] = 2.0 * (n[2] * Y[1] - n[1] * Y[2]);
  c[2] = 2.0 * (n[0] * Y[2] - n[2] * Y[0]);
  c[3] = 2.0 * (n[1] * Y[0] - n[0] * Y[1]);
  c[4] = (d0 - d1) - d2;
  c[5] = 2.0 * (n[0] * Y[1] + n[1] * Y[0]);
  c[6] = 2.0 * (n[0] * Y[2] + n[2] * Y[0]);
  c[7] = (d1 - d0) - d2;
  c[8] = 2.0 * (n[1] * Y[2] + n[2] * Y[1]);
  c[9] = (d2 - d0) - d1;
}

// u, v spanning the plane orthogonal to x: u = x cross e_k normalised, k the smallest |x_k| (the first on ties),
// v = x cross u
LT_HD bool es_plane_basis(const double x[3], double u[3], double v[3]) {
  int k = 0;
  if (es_abs(x[1]) < es_abs(x[k])) k = 1;
  if (es_abs(x[2]) < es_abs(x[k])) k = 2;
  double e[3] = {0.0, 0.0, 0.0};
  e[k] = 1.0;
  u[0] = x[1] * e[2] - x[2] * e[1];
  u[1] = x[2] * e[0] - x[0] * e[2];
  u[2] = x[0] * e[1] - x[1] * e[0];
  const double len = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  if (!(len > 0.0)) return false;
  for (int c = 0; c < 3; ++c) u[c] = u[c] / len;
  v[0] = x[1] * u[2] - x[2] * u[1];
  v[1] = x[2] * u[0] - x[0] * u[2];
  v[2] = x[0] * u[1] - x[1] * u[0];
  return true;
}

// out[i + j] += s a[i] b[j]
LT_HD void es_pmac(double *out, double s, const double *a, int da, const double *b, int db) {
  for (int i = 0; i <= da; ++i)
    for (int j = 0; j <= db; ++j) out[i + j] = out[i + j] + s * (a[i] * b[j]);
}

LT_HD double es_horner(const double *p, int deg, double z) {
  double v = p[deg];
  for (int i = deg - 1; i >= 0; --i) v = v * z + p[i];
  return v;
}

// The polynomials x2, xy, y2 = P[k][0] x + P[k][1] y + P[k][2] of the solved constant block (degrees 1, 1, 2 in z);
// a x2 + b xy + c y2 + lx x + ly y + lc, with a, b, c of degree da, reduced to [x, y, 1]: out[3][5]
LT_HD void es_subst(const double P[3][3][3], const double *a, const double *b, const double *c, int da, const double *lx,
                    const double *ly, int dl, const double *lc, int dc, double out[3][5]) {
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 5; ++i) out[j][i] = 0.0;
  for (int j = 0; j < 3; ++j) {
    const int dp = j == 2 ? 2 : 1;
    es_pmac(out[j], 1.0, a, da, P[0][j], dp);
    es_pmac(out[j], 1.0, b, da, P[1][j], dp);
    es_pmac(out[j], 1.0, c, da, P[2][j], dp);
  }
  for (int i = 0; i <= dl; ++i) {
    out[0][i] = out[0][i] + lx[i];
    out[1][i] = out[1][i] + ly[i];
  }
  for (int i = 0; i <= dc; ++i) out[2][i] = out[2][i] + lc[i];
}

// The real roots of the octic p (ascending coefficients), ascending in roots[]: a Sturm chain (every member scaled to
// max-abs 1, a remainder cut where its coefficients fall below kEsChainTol), the k-th root bracketed by kEsBisect
// bisections inside the Cauchy bound -- on the chain's sign changes until the root is alone in its interval, then on the
// sign of p -- and kEsRootNewton Newton steps on p.
ES_HD int es_octic_roots(const double p[9], double roots[8]) {
  double amax = 0.0;
  for (int i = 0; i <= 8; ++i) {
    if (!es_finite(p[i])) return 0;
    if (es_abs(p[i]) > amax) amax = es_abs(p[i]);
  }
  if (!(amax > 0.0) || !(es_abs(p[8]) > kEsLeadTol * amax)) return 0;
  double ch[9][9];
  int dg[9];
  double bound = 0.0;
  for (int i = 0; i <= 8; ++i) ch[0][i] = p[i] / p[8];
  for (int i = 0; i < 8; ++i)
    if (es_abs(ch[0][i]) > bound) bound = es_abs(ch[0][i]);
  bound = 1.0 + bound;
  double der[8];  // the derivative of the monic octic
  for (int i = 0; i < 8; ++i) der[i] = (double)(i + 1) * ch[0][i + 1];
  double mono[9];
  for (int i = 0; i <= 8; ++i) mono[i] = ch[0][i];
  {
    double s = 0.0;
    for (int i = 0; i <= 8; ++i)
      if (es_abs(ch[0][i]) > s) s = es_abs(ch[0][i]);
    for (int i = 0; i <= 8; ++i) ch[0][i] = ch[0][i] / s;
    s = 0.0;
    for (int i = 0; i < 8; ++i)
      if (es_abs(der[i]) > s) s = es_abs(der[i]);
    for (int i = 0; i < 8; ++i) ch[1][i] = der[i] / s;
    ch[1][8] = 0.0;
  }
  dg[0] = 8;
  dg[1] = 7;
  int nch = 2;
  for (; nch < 9; ++nch) {
    // remainder of ch[nch - 2] by ch[nch - 1], negated
    double r[9];
    const int da = dg[nch - 2], db = dg[nch - 1];
    if (db == 0) break;
    for (int i = 0; i <= 8; ++i) r[i] = i <= da ? ch[nch - 2][i] : 0.0;
    for (int k = da; k >= db; --k) {
      const double f = r[k] / ch[nch - 1][db];
      for (int j = 0; j <= db; ++j) r[k - db + j] = r[k - db + j] - f * ch[nch - 1][j];
      r[k] = 0.0;
    }
    double rmax = 0.0;
    for (int i = 0; i < db; ++i)
      if (es_abs(r[i]) > rmax) rmax = es_abs(r[i]);
    if (!(rmax > kEsChainTol)) break;  // a common factor: the chain ends (a multiple root counts once)
    int d = db - 1;
    while (d > 0 && !(es_abs(r[d]) > kEsChainTol * rmax)) --d;
    for (int i = 0; i <= 8; ++i) ch[nch][i] = i <= d ? -(r[i] / rmax) : 0.0;
    dg[nch] = d;
  }
  // sign changes of the chain at z
  auto changes = [&](double z) {
    int n = 0, last = 0;
    for (int k = 0; k < nch; ++k) {
      const double v = es_horner(ch[k], dg[k], z);
      const int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
      if (s != 0) {
        if (last != 0 && s != last) ++n;
        last = s;
      }
    }
    return n;
  };
  const int c_lo = changes(-bound);
  int n_roots = c_lo - changes(bound);
  if (n_roots <= 0) return 0;
  if (n_roots > 8) n_roots = 8;
  int out = 0;
  for (int k = 1; k <= n_roots; ++k) {
    double lo = -bound, hi = bound;
    int n_lo = 0, n_hi = n_roots, it = 0;  // roots in (-bound, lo] and in (-bound, hi]: n_lo < k <= n_hi
    for (; it < kEsBisect && n_hi - n_lo != 1; ++it) {
      const double mid = 0.5 * (lo + hi);
      const int c = c_lo - changes(mid);
      if (c >= k) { hi = mid; n_hi = c; } else { lo = mid; n_lo = c; }
    }
    // the root is alone in (lo, hi]: where p changes its sign over the interval, the remaining bisections look at the
    // sign of p only (one evaluation instead of the chain's nine)
    const double f_lo = es_horner(mono, 8, lo), f_hi = es_horner(mono, 8, hi);
    const bool by_sign = (f_lo < 0.0 && f_hi > 0.0) || (f_lo > 0.0 && f_hi < 0.0);
    for (; it < kEsBisect; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (by_sign) {
        const double f = es_horner(mono, 8, mid);
        if (f == 0.0) { lo = mid; hi = mid; }
        else if ((f < 0.0) == (f_lo < 0.0)) lo = mid;
        else hi = mid;
      } else if (c_lo - changes(mid) >= k) {
        hi = mid;
      } else {
        lo = mid;
      }
    }
    // Newton inside the bracket: a step that leaves [lo, hi] ends the refinement, so the roots stay in ascending order
    double z = 0.5 * (lo + hi);
    for (int nw = 0; nw < kEsRootNewton; ++nw) {
      const double f = es_horner(mono, 8, z), d = es_horner(der, 7, z);
      if (d == 0.0) break;
      const double zn = z - f / d;
      if (!(zn >= lo && zn <= hi)) break;
      z = zn;
    }
    roots[out++] = z;
  }
  return out;
}

// Gaussian elimination with partial pivoting of the n x n system A u = b (A, b overwritten); false where a pivot is not
// above tol times the largest entry of A
template <int N>
LT_HD bool es_gauss(double A[N][N], double b[N], double u[N], double tol) {
  double amax = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j)
      if (es_abs(A[i][j]) > amax) amax = es_abs(A[i][j]);
  if (!(amax > 0.0) || !es_finite(amax)) return false;
  for (int k = 0; k < N; ++k) {
    int piv = k;
    for (int i = k + 1; i < N; ++i)
      if (es_abs(A[i][k]) > es_abs(A[piv][k])) piv = i;
    if (!(es_abs(A[piv][k]) > tol * amax)) return false;
    if (piv != k) {
      for (int j = 0; j < N; ++j) { const double s = A[k][j]; A[k][j] = A[piv][j]; A[piv][j] = s; }
      const double s = b[k]; b[k] = b[piv]; b[piv] = s;
    }
    for (int i = k + 1; i < N; ++i) {
      const double f = A[i][k] / A[k][k];
      for (int j = k; j < N; ++j) A[i][j] = A[i][j] - f * A[k][j];
      b[i] = b[i] - f * b[k];
    }
  }
  for (int i = N - 1; i >= 0; --i) {
    double s = b[i];
    for (int j = i + 1; j < N; ++j) s = s - A[i][j] * u[j];
    u[i] = s / A[i][i];
  }
  return true;
}

// CameraPose::R() of a unit quaternion (base/pose.cc)
LT_HD void es_rotation(const double q[4], double R[3][3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
}

// the monomials in the chart w = 1
LT_HD void es_chart_monomials(double x, double y, double z, double m[10]) {
  m[0] = 1.0; m[1] = x; m[2] = y; m[3] = z;
  m[4] = x * x; m[5] = x * y; m[6] = x * z; m[7] = y * y; m[8] = y * z; m[9] = z * z;
}

// One sample -> up to kEsMaxSol poses (qvec normalised with w > 0, tvec), in ascending order of the root z / w.
// x X: np x 3; l C V: (3 - np) x 3.
ES_HD int es_solve(int np, const double x[3][3], const double X[3][3], const double l[3][3], const double C[3][3],
                   const double V[3][3], double poses[kEsMaxSol][kEsPoseDoubles]) {
  if (np < 0 || np > 3) return 0;
  const int nl = 3 - np, m = 2 * np + nl;
  // raw[r] = n (3, times sigma) | c (10): the six constraints, the sigma = 1 rows first
  double raw[6][13];
  double nrm[6][3];  // the normals of all six rows (the residual test)
  {
    int r = 0;
    for (int i = 0; i < np; ++i) {
      double u[3], v[3];
      if (!es_plane_basis(x[i], u, v)) return 0;
      for (int c = 0; c < 3; ++c) { raw[r][c] = u[c]; raw[r + 1][c] = v[c]; }
      es_quad_row(u, X[i], raw[r] + 3);
      es_quad_row(v, X[i], raw[r + 1] + 3);
      r += 2;
    }
    for (int j = 0; j < nl; ++j, ++r) {
      for (int c = 0; c < 3; ++c) raw[r][c] = l[j][c];
      es_quad_row(l[j], C[j], raw[r] + 3);
    }
    for (int j = 0; j < nl; ++j, ++r) {
      for (int c = 0; c < 3; ++c) raw[r][c] = 0.0;
      es_quad_row(l[j], V[j], raw[r] + 3);
    }
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 3; ++c) nrm[rr][c] = rr < m ? raw[rr][c] : l[rr - m][c];
  }
  // Householder triangularisation of the normals, applied to the whole rows
  double A[6][13];
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < 13; ++c) A[r][c] = raw[r][c];
  for (int k = 0; k < 3; ++k) {
    double s2 = 0.0;
    for (int i = k; i < m; ++i) s2 = s2 + A[i][k] * A[i][k];
    const double alpha = sqrt(s2);
    if (!(alpha > kEsRankTol)) return 0;  // the normals do not span the translation
    double v[6];
    for (int i = k; i < m; ++i) v[i] = A[i][k];
    v[k] = v[k] + (A[k][k] < 0.0 ? -alpha : alpha);
    double vn = 0.0;
    for (int i = k; i < m; ++i) vn = vn + v[i] * v[i];
    if (!(vn > 0.0)) return 0;
    for (int j = k; j < 13; ++j) {
      double d = 0.0;
      for (int i = k; i < m; ++i) d = d + v[i] * A[i][j];
      const double f = 2.0 * d / vn;
      for (int i = k; i < m; ++i) A[i][j] = A[i][j] - f * v[i];
    }
  }
  // the three quadrics, each scaled to max-abs 1
  double E[3][10];
  for (int e = 0; e < 3; ++e) {
    const double *src = e < m - 3 ? A[3 + e] + 3 : raw[m + (e - (m - 3))] + 3;
    double s = 0.0;
    for (int c = 0; c < 10; ++c)
      if (es_abs(src[c]) > s) s = es_abs(src[c]);
    if (!(s > 0.0) || !es_finite(s)) return 0;
    for (int c = 0; c < 10; ++c) E[e][c] = src[c] / s;
  }
  // x2, xy, y2 from the constant block: G [x2 xy y2]^T = -(columns xz wx yz wy z2 wz w2)
  double S[3][7];
  {
    const int gcol[3] = {4, 5, 7}, rcol[7] = {6, 1, 8, 2, 9, 3, 0};
    double G[3][10];
    for (int e = 0; e < 3; ++e) {
      for (int c = 0; c < 3; ++c) G[e][c] = E[e][gcol[c]];
      for (int c = 0; c < 7; ++c) G[e][3 + c] = -E[e][rcol[c]];
    }
    for (int k = 0; k < 3; ++k) {
      int piv = k;
      for (int i = k + 1; i < 3; ++i)
        if (es_abs(G[i][k]) > es_abs(G[piv][k])) piv = i;
      if (!(es_abs(G[piv][k]) > kEsPivotTol)) return 0;  // singular constant block
      if (piv != k)
        for (int j = 0; j < 10; ++j) { const double s = G[k][j]; G[k][j] = G[piv][j]; G[piv][j] = s; }
      for (int i = 0; i < 3; ++i) {
        if (i == k) continue;
        const double f = G[i][k] / G[k][k];
        for (int j = k; j < 10; ++j) G[i][j] = G[i][j] - f * G[k][j];
      }
    }
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 7; ++c) S[k][c] = G[k][3 + c] / G[k][k];
  }
  // P[k][0] on x, P[k][1] on y (degree 1), P[k][2] constant (degree 2), ascending in z
  double P[3][3][3];
  for (int k = 0; k < 3; ++k) {
    P[k][0][0] = S[k][1]; P[k][0][1] = S[k][0]; P[k][0][2] = 0.0;
    P[k][1][0] = S[k][3]; P[k][1][1] = S[k][2]; P[k][1][2] = 0.0;
    P[k][2][0] = S[k][6]; P[k][2][1] = S[k][5]; P[k][2][2] = S[k][4];
  }
  // the identities x (xy) = y (x2), y (xy) = x (y2), (x2)(y2) = (xy)^2 reduced to [x, y, 1]: M[row][col], degrees
  // (2, 2, 3), (2, 2, 3), (3, 3, 4)
  double M[3][3][5];
  {
    double a[5], b[5], c[5], lx[5], ly[5], lc[5];
    // x (xy) - y (x2)
    for (int i = 0; i < 2; ++i) { a[i] = P[1][0][i]; b[i] = P[1][1][i] - P[0][0][i]; c[i] = -P[0][1][i]; }
    for (int i = 0; i < 3; ++i) { lx[i] = P[1][2][i]; ly[i] = -P[0][2][i]; }
    lc[0] = 0.0;
    es_subst(P, a, b, c, 1, lx, ly, 2, lc, 0, M[0]);
    // y (xy) - x (y2)
    for (int i = 0; i < 2; ++i) { a[i] = -P[2][0][i]; b[i] = P[1][0][i] - P[2][1][i]; c[i] = P[1][1][i]; }
    for (int i = 0; i < 3; ++i) { lx[i] = -P[2][2][i]; ly[i] = P[1][2][i]; }
    es_subst(P, a, b, c, 1, lx, ly, 2, lc, 0, M[1]);
    // (x2)(y2) - (xy)^2
    for (int i = 0; i < 5; ++i) a[i] = b[i] = c[i] = lx[i] = ly[i] = lc[i] = 0.0;
    es_pmac(a, 1.0, P[0][0], 1, P[2][0], 1);
    es_pmac(a, -1.0, P[1][0], 1, P[1][0], 1);
    es_pmac(b, 1.0, P[0][0], 1, P[2][1], 1);
    es_pmac(b, 1.0, P[0][1], 1, P[2][0], 1);
    es_pmac(b, -2.0, P[1][0], 1, P[1][1], 1);
    es_pmac(c, 1.0, P[0][1], 1, P[2][1], 1);
    es_pmac(c, -1.0, P[1][1], 1, P[1][1], 1);
    es_pmac(lx, 1.0, P[0][0], 1, P[2][2], 2);
    es_pmac(lx, 1.0, P[0][2], 2, P[2][0], 1);
    es_pmac(lx, -2.0, P[1][0], 1, P[1][2], 2);
    es_pmac(ly, 1.0, P[0][1], 1, P[2][2], 2);
    es_pmac(ly, 1.0, P[0][2], 2, P[2][1], 1);
    es_pmac(ly, -2.0, P[1][1], 1, P[1][2], 2);
    es_pmac(lc, 1.0, P[0][2], 2, P[2][2], 2);
    es_pmac(lc, -1.0, P[1][2], 2, P[1][2], 2);
    es_subst(P, a, b, c, 2, lx, ly, 3, lc, 4, M[2]);
  }
  // the determinant: expansion along the first row, minors of rows 1 and 2
  double det[9];
  {
    const int dr[3][3] = {{2, 2, 3}, {2, 2, 3}, {3, 3, 4}};
    double acc[13];
    for (int i = 0; i < 13; ++i) acc[i] = 0.0;
    const int cols[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    for (int j = 0; j < 3; ++j) {
      const int c0 = cols[j][0], c1 = cols[j][1];
      double mn[9];
      for (int i = 0; i < 9; ++i) mn[i] = 0.0;
      es_pmac(mn, 1.0, M[1][c0], dr[1][c0], M[2][c1], dr[2][c1]);
      es_pmac(mn, -1.0, M[1][c1], dr[1][c1], M[2][c0], dr[2][c0]);
      const int dm = (dr[1][c0] + dr[2][c1]) > (dr[1][c1] + dr[2][c0]) ? (dr[1][c0] + dr[2][c1]) : (dr[1][c1] + dr[2][c0]);
      es_pmac(acc, j == 1 ? -1.0 : 1.0, M[0][j], dr[0][j], mn, dm);
    }
    for (int i = 0; i < 9; ++i) det[i] = acc[i];
  }
  double roots[8];
  const int n_roots = es_octic_roots(det, roots);
  int n_out = 0;
  for (int ri = 0; ri < n_roots && n_out < kEsMaxSol; ++ri) {
    double z = roots[ri];
    // (x, y, 1): the null vector of M(z), the cross product of the two rows (each scaled to max-abs 1) that gives the
    // longest one
    double Mn[3][3];
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
      double s = 0.0;
      for (int j = 0; j < 3; ++j) {
        Mn[i][j] = es_horner(M[i][j], 4, z);
        if (es_abs(Mn[i][j]) > s) s = es_abs(Mn[i][j]);
      }
      if (!es_finite(s)) ok = false;
      if (s > 0.0)
        for (int j = 0; j < 3; ++j) Mn[i][j] = Mn[i][j] / s;
    }
    if (!ok) continue;
    double best[3] = {0.0, 0.0, 0.0}, best_n = -1.0;
    const int pr[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int k = 0; k < 3; ++k) {
      const double *a = Mn[pr[k][0]], *b = Mn[pr[k][1]];
      const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
      const double n2 = (cx * cx + cy * cy) + cz * cz;
      if (n2 > best_n) { best_n = n2; best[0] = cx; best[1] = cy; best[2] = cz; }
    }
    if (!(best_n > 0.0) || !(best[2] * best[2] > 1e-24 * best_n)) continue;  // no affine null vector
    double xx = best[0] / best[2], yy = best[1] / best[2];
    // t' from the triangular rows: R t' = -(c . monomials)
    double tp[3];
    {
      double mon[10];
      es_chart_monomials(xx, yy, z, mon);
      for (int i = 2; i >= 0; --i) {
        double s = 0.0;
        for (int c = 0; c < 10; ++c) s = s + A[i][3 + c] * mon[c];
        s = -s;
        for (int j = i + 1; j < 3; ++j) s = s - A[i][j] * tp[j];
        tp[i] = s / A[i][i];
      }
    }
    // Newton on the six constraints in (x, y, z, t')
    for (int it = 0; it < kEsPolish; ++it) {
      double J[6][6], F[6], du[6], mon[10];
      es_chart_monomials(xx, yy, z, mon);
      const double dx[10] = {0.0, 1.0, 0.0, 0.0, 2.0 * xx, yy, z, 0.0, 0.0, 0.0};
      const double dy[10] = {0.0, 0.0, 1.0, 0.0, 0.0, xx, 0.0, 2.0 * yy, z, 0.0};
      const double dz[10] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, xx, 0.0, yy, 2.0 * z};
      for (int r = 0; r < 6; ++r) {
        double f = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
        for (int c = 0; c < 10; ++c) {
          f = f + raw[r][3 + c] * mon[c];
          jx = jx + raw[r][3 + c] * dx[c];
          jy = jy + raw[r][3 + c] * dy[c];
          jz = jz + raw[r][3 + c] * dz[c];
        }
        for (int c = 0; c < 3; ++c) {
          f = f + raw[r][c] * tp[c];
          J[r][3 + c] = raw[r][c];
        }
        J[r][0] = jx; J[r][1] = jy; J[r][2] = jz;
        F[r] = -f;
      }
      if (!es_gauss<6>(J, F, du, kEsNewtonTol)) break;
      bool fin = true;
      for (int c = 0; c < 6; ++c) fin = fin && es_finite(du[c]);
      if (!fin) break;
      xx = xx + du[0]; yy = yy + du[1]; z = z + du[2];
      for (int c = 0; c < 3; ++c) tp[c] = tp[c] + du[3 + c];
    }
    const double n2 = ((1.0 + xx * xx) + yy * yy) + z * z;
    const double nq = sqrt(n2);
    double q[4] = {1.0 / nq, xx / nq, yy / nq, z / nq};
    double t[3] = {tp[0] / n2, tp[1] / n2, tp[2] / n2};
    bool fin = es_finite(n2);
    for (int c = 0; c < 4; ++c) fin = fin && es_finite(q[c]);
    for (int c = 0; c < 3; ++c) fin = fin && es_finite(t[c]);
    if (!fin) continue;
    double R[3][3];
    es_rotation(q, R);
    // the six constraints as sines of angles, and the point depths
    for (int r = 0; r < 6 && ok; ++r) {
      const double *Y = r < 2 * np ? X[r / 2] : (r < m ? C[r - 2 * np] : V[r - m]);
      const double sg = r < m ? 1.0 : 0.0;
      double w[3];
      for (int c = 0; c < 3; ++c) w[c] = ((R[c][0] * Y[0] + R[c][1] * Y[1]) + R[c][2] * Y[2]) + sg * t[c];
      const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
      if (!(len > 0.0)) { ok = false; break; }
      const double res = es_abs((nrm[r][0] * w[0] + nrm[r][1] * w[1]) + nrm[r][2] * w[2]) / len;
      if (!(res <= kEsResidualTol)) { ok = false; break; }
      if (r < 2 * np && (r & 1) == 0) {
        const double *b = x[r / 2];
        if (!((b[0] * w[0] + b[1] * w[1]) + b[2] * w[2] > 0.0)) { ok = false; break; }
      }
    }
    if (!ok) continue;
    for (int c = 0; c < 4; ++c) poses[n_out][c] = q[c];
    for (int c = 0; c < 3; ++c) poses[n_out][4 + c] = t[c];
    ++n_out;
  }
  return n_out;
}

// the sample table of a batch: field f of sample i at tab[f * stride + i]; fields x X l C V, each 3 x 3
struct EsDev {
  const double *tab;
  long long stride;
  long long n;
  int kind;
  int pad_;
};

LT_HD void es_load(const EsDev &d, long long i, double x[3][3], double X[3][3], double l[3][3], double C[3][3],
                   double V[3][3]) {
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) {
      const int f = 3 * a + c;
      x[a][c] = d.tab[(long long)f * d.stride + i];
      X[a][c] = d.tab[(long long)(9 + f) * d.stride + i];
      l[a][c] = d.tab[(long long)(18 + f) * d.stride + i];
      C[a][c] = d.tab[(long long)(27 + f) * d.stride + i];
      V[a][c] = d.tab[(long long)(36 + f) * d.stride + i];
    }
}

void launch_est_minimal(hipStream_t st, const EsDev &dev, double *poses, int *counts);

}  // namespace lt
