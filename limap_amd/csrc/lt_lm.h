// lt_lm.h -- the numerical core the minimisers of lt_refine.h, lt_loc.h, lt_ba.h and lt_assoc.h share: the
// forward-mode scalar, the damped step, the trust-region loop over a chart, the xor trees of the reductions, the chunked
// reduction and the block pieces of the coupled solves, and the rotation, the line projection and the quaternion
// normalisation more than one of them evaluates.  Every definition here is a
// bit-exactness contract -- the device equals its host twin bit for bit, and both equal the NumPy restatements of the
// tests -- so each exists once: a new minimiser uses these, it does not bring its own.  Both sides compile them with
// -ffp-contract=off.
#pragma once

#include "lt_geom.h"

namespace lt {

// ---- the minimiser's constants and termination codes ----
constexpr double kRfMu0 = 1e4;          // initial trust-region radius (Ceres' default)
constexpr double kRfMuMax = 1e16, kRfMuMin = 1e-32;
constexpr double kRfMinRatio = 1e-3;    // min_relative_decrease
constexpr double kRfDMin = 1e-6, kRfDMax = 1e32;  // min / max_lm_diagonal

enum RfCode : int {
  kRfMaxIter = 0,    // max_num_iterations reached
  kRfRadius = 1,     // the radius fell below 1e-32
  kRfZeroGrad = 2,   // g == 0
  kRfBadPivot = 3,   // a Cholesky pivot is not positive or not finite
  kRfBadModel = 4,   // the model decrease is not positive or not finite
  kRfConstant = 5,   // constant_line, or fewer than min_num_images images: not optimised, segment re-cut
  kRfEvalFailed = 6, // the cost at the initial point is not finite (a heatmap sample failed): not optimised, segment re-cut
};

LT_HD double lt_exp(double x);  // lt_refine.h

// ---- forward-mode scalar: a value and its derivatives along N local directions.  The rules are Ceres' Jet's, with
// d|x|/dx = +1 at x = 0; a double converts to the constant (all derivatives 0) ----
template <int N>
struct Jet {
  double v, d[N];
  Jet() = default;
  LT_HD Jet(double x) : v(x) {
    for (int i = 0; i < N; ++i) d[i] = 0.0;
  }
};
#define LT_JET template <int N> LT_HD Jet<N>
LT_JET operator+(const Jet<N> &a, const Jet<N> &b) { Jet<N> r; r.v = a.v + b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
LT_JET operator-(const Jet<N> &a, const Jet<N> &b) { Jet<N> r; r.v = a.v - b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
LT_JET operator-(const Jet<N> &a) { Jet<N> r; r.v = -a.v; for (int i = 0; i < N; ++i) r.d[i] = -a.d[i]; return r; }
LT_JET operator*(const Jet<N> &a, const Jet<N> &b) { Jet<N> r; r.v = a.v * b.v; for (int i = 0; i < N; ++i) r.d[i] = a.v * b.d[i] + a.d[i] * b.v; return r; }
LT_JET operator/(const Jet<N> &a, const Jet<N> &b) { Jet<N> r; r.v = a.v / b.v; for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v; return r; }
LT_JET operator+(const Jet<N> &a, double b) { Jet<N> r = a; r.v = a.v + b; return r; }
LT_JET operator+(double b, const Jet<N> &a) { Jet<N> r = a; r.v = b + a.v; return r; }
LT_JET operator-(const Jet<N> &a, double b) { Jet<N> r = a; r.v = a.v - b; return r; }
LT_JET operator-(double b, const Jet<N> &a) { Jet<N> r; r.v = b - a.v; for (int i = 0; i < N; ++i) r.d[i] = -a.d[i]; return r; }
LT_JET operator*(const Jet<N> &a, double b) { Jet<N> r; r.v = a.v * b; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b; return r; }
LT_JET operator*(double b, const Jet<N> &a) { return a * b; }
LT_JET operator/(const Jet<N> &a, double b) { Jet<N> r; r.v = a.v / b; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] / b; return r; }
LT_JET operator/(double a, const Jet<N> &b) { Jet<N> r; r.v = a / b.v; for (int i = 0; i < N; ++i) r.d[i] = (-(r.v * b.d[i])) / b.v; return r; }
LT_JET rf_sqrt(const Jet<N> &a) { Jet<N> r; r.v = sqrt(a.v); const double h = 0.5 / r.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * h; return r; }
LT_JET rf_abs(const Jet<N> &a) { return a.v < 0.0 ? -a : a; }
LT_JET rf_exp(const Jet<N> &a) { Jet<N> r; r.v = lt_exp(a.v); for (int i = 0; i < N; ++i) r.d[i] = r.v * a.d[i]; return r; }
LT_JET rf_inv(const Jet<N> &a) { return 1.0 / a; }
#undef LT_JET
template <int N> LT_HD double rf_val(const Jet<N> &a) { return a.v; }
template <int N> LT_HD void rf_set(Jet<N> &a, double v) { a = Jet<N>(v); }
// the same names over a plain double, so that one template serves the cost (double) and the linearisation (a jet)
LT_HD double rf_sqrt(double a) { return sqrt(a); }
LT_HD double rf_abs(double a) { return a < 0.0 ? -a : a; }
LT_HD double rf_exp(double a) { return lt_exp(a); }
LT_HD double rf_inv(double a) { return 1.0 / a; }
LT_HD double rf_val(double a) { return a; }
LT_HD void rf_set(double &a, double v) { a = v; }

// the quaternion q and its first three local directions (0, e_i) (x) q; the further derivatives are 0
template <int N>
LT_HD void lm_seed_quat(const double q[4], Jet<N> u[4]) {
  for (int i = 0; i < 4; ++i) u[i] = Jet<N>(q[i]);
  u[0].d[0] = -q[1]; u[0].d[1] = -q[2]; u[0].d[2] = -q[3];
  u[1].d[0] = q[0];  u[1].d[1] = q[3];  u[1].d[2] = -q[2];
  u[2].d[0] = -q[3]; u[2].d[1] = q[0];  u[2].d[2] = q[1];
  u[3].d[0] = q[2];  u[3].d[1] = -q[1]; u[3].d[2] = q[0];
}

// the quaternion part of a retraction: out = normalize((1, dq) (x) q)
LT_HD void lm_retract_quat(const double q[4], const double dq[3], double out[4]) {
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  const double r0 = ((q0 - dq[0] * q1) - dq[1] * q2) - dq[2] * q3;
  const double r1 = ((q1 + dq[0] * q0) + dq[1] * q3) - dq[2] * q2;
  const double r2 = ((q2 - dq[0] * q3) + dq[1] * q0) + dq[2] * q1;
  const double r3 = ((q3 + dq[0] * q2) - dq[1] * q1) + dq[2] * q0;
  const double nu = sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
  out[0] = r0 / nu; out[1] = r1 / nu; out[2] = r2 / nu; out[3] = r3 / nu;
}

// ---- the damped step ----
// the sums of a linearisation with N unknowns, in the order every reduction uses: the upper triangle of H by rows
// (00 01 .. 0(N-1) 11 ..), then g
constexpr int lm_sums(int n) { return n * (n + 1) / 2 + n; }

// the damped diagonal entry h + D^2 / mu, D = clamp(sqrt h, 1e-6, 1e32), and the test of a Cholesky pivot
LT_HD double lm_damp(double h, double mu) {
  double dg = sqrt(h);
  dg = dg < kRfDMin ? kRfDMin : (dg > kRfDMax ? kRfDMax : dg);
  return h + (dg * dg) / mu;
}
LT_HD bool lm_pivot_ok(double v) { return v > 0.0 && v < kMaxDist; }

// the Levenberg-Marquardt step from the reduced sums: (H + D^2 / mu) dl = -g by an N x N Cholesky factorisation.
// Returns 0, or the termination code; md = the model decrease -(g' dl + dl' H dl / 2)
template <int N>
LT_HD int lm_step(const double acc[lm_sums(N)], double mu, double dl[N], double *md) {
  double H[N][N], L[N][N], y[N];
  int o = 0;
  for (int i = 0; i < N; ++i)
    for (int j = i; j < N; ++j, ++o) H[i][j] = H[j][i] = acc[o];
  const double *g = acc + N * (N + 1) / 2;
  for (int i = 0; i < N; ++i) {
    const double hii = lm_damp(H[i][i], mu);
    for (int j = 0; j <= i; ++j) {
      double sum = i == j ? hii : H[i][j];
      for (int k = 0; k < j; ++k) sum = sum - L[i][k] * L[j][k];
      if (i == j) {
        if (!lm_pivot_ok(sum)) return kRfBadPivot;
        L[i][i] = sqrt(sum);
      } else {
        L[i][j] = sum / L[j][j];
      }
    }
  }
  for (int i = 0; i < N; ++i) {
    double sum = -g[i];
    for (int k = 0; k < i; ++k) sum = sum - L[i][k] * y[k];
    y[i] = sum / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double sum = y[i];
    for (int k = i + 1; k < N; ++k) sum = sum - L[k][i] * dl[k];
    dl[i] = sum / L[i][i];
  }
  double gd = 0.0, dhd = 0.0;
  for (int i = 0; i < N; ++i) {
    gd = gd + g[i] * dl[i];
    double hd = 0.0;
    for (int j = 0; j < N; ++j) hd = hd + H[i][j] * dl[j];
    dhd = dhd + dl[i] * hd;
  }
  *md = -(gd + 0.5 * dhd);
  if (!(*md > 0.0) || !(*md < kMaxDist)) return kRfBadModel;
  return 0;
}

// the radius after an accepted step
LT_HD double rf_grow(double mu, double ratio) {
  const double t = 2.0 * ratio - 1.0;
  double f = 1.0 - (t * t) * t;
  f = f < 1.0 / 3.0 ? 1.0 / 3.0 : f;
  const double m = mu / f;
  return m < kRfMuMax ? m : kRfMuMax;
}

// ---- the trust-region loop from the point p with the cost F = grp.cost(p).  A chart supplies
//   kParams                 the doubles of a point
//   kStep                   the unknowns of a step: grp.linearise(p, acc) fills lm_sums(kStep) sums
//   retract(p, dl, out)     the point a step leads to
// G supplies the two reductions -- cost(p) and linearise(p, acc) -- as values every lane of a group holds bit for bit
// (device: lm_group_sum; host: lm_tree_host), so every branch below is uniform over the group.  An iteration counts
// whether its step was accepted or not.  What a caller checks before the loop (a constant track, a start that is not
// finite, a problem without residuals) is the caller's, in the caller's order ----
template <class Chart, class G>
LT_HD void lm_loop(G &grp, double F, int max_iter, double *p, double *cost1, int *iters, int *code_out) {
  constexpr int NS = Chart::kStep, NP = Chart::kParams;
  int it = 0, code = kRfMaxIter;
  double mu = kRfMu0, nu = 2.0;
  double acc[lm_sums(NS)];
  bool fresh = true;
  for (; it < max_iter; ++it) {
    if (fresh) {
      grp.linearise(p, acc);
      bool zero = true;
      for (int c = 0; c < NS; ++c) zero = zero && acc[NS * (NS + 1) / 2 + c] == 0.0;
      if (zero) { code = kRfZeroGrad; break; }
      fresh = false;
    }
    double dl[NS], md;
    const int rc = lm_step<NS>(acc, mu, dl, &md);
    if (rc) { code = rc; break; }
    double pn[NP];
    Chart::retract(p, dl, pn);
    const double Fn = grp.cost(pn);
    const double ratio = (F - Fn) / md;
    if (ratio > kRfMinRatio) {
      for (int c = 0; c < NP; ++c) p[c] = pn[c];
      F = Fn;
      mu = rf_grow(mu, ratio);
      nu = 2.0;
      fresh = true;
    } else {
      mu = mu / nu;
      nu = 2.0 * nu;
      if (mu < kRfMuMin) { code = kRfRadius; ++it; break; }
    }
  }
  *cost1 = F;
  *iters = it;
  *code_out = code;
}
// the end of a solve that does not enter the loop
LT_HD void lm_skip(double F, int code, double *cost1, int *iters, int *code_out) {
  *cost1 = F;
  *iters = 0;
  *code_out = code;
}

// ---- the fixed xor tree over W partial sums: m = W/2 .. 1 with v + v[l ^ m], so that every lane holds the same bits
// (a + b == b + a).  Host: part[l] holds lane l's sums, the first n of them are reduced ----
template <int W, int C>
inline void lm_tree_host(double (&part)[W][C], int n, double *out) {
  static_assert(W > 0 && (W & (W - 1)) == 0, "a group is a power of two of lanes");
  for (int m = W / 2; m >= 1; m >>= 1) {
    double nxt[W][C];
    for (int l = 0; l < W; ++l)
      for (int c = 0; c < n; ++c) nxt[l][c] = part[l][c] + part[l ^ m][c];
    for (int l = 0; l < W; ++l)
      for (int c = 0; c < n; ++c) part[l][c] = nxt[l][c];
  }
  for (int c = 0; c < n; ++c) out[c] = part[0][c];
}
#ifdef __HIPCC__
// device: the sum over the W lanes of a group (W a power of two up to the wave's 64)
template <int W>
__device__ __forceinline__ double lm_group_sum(double v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, W);
  return v;
}
#endif

// ---- the lanes of a group: what a minimiser's group is written over, once for the wave and its host twin.
//   sum<C>(n, part, out)          part(l, acc) adds lane l's terms to its acc[C], zeroed before; the first n sums are
//                                 reduced by the xor tree into out (C doubles), which every lane then holds
//   over<C>(n_items, n, item, out)  the same with item(i, acc) for the lane's items i = l, l + W, ... in ascending order;
//                                 over<C, S>: the items go to the first S lanes (i = l, l + S, ...), the others add zeros
//   lead(), sync()                the lane that writes what the group shares, and the barrier around such writes
// Host: the lanes are a loop ----
template <int W>
struct LmHostLanes {
  bool lead() const { return true; }
  void sync() const {}
  template <int C, class F>
  void sum(int n, F part, double *out) const {
    double acc[W][C];
    for (int l = 0; l < W; ++l) {
      for (int c = 0; c < C; ++c) acc[l][c] = 0.0;
      part(l, acc[l]);
    }
    lm_tree_host(acc, n, out);
  }
  template <int C, int S = W, class I, class F>
  void over(I n_items, int n, F item, double *out) const {
    sum<C>(n, [&](int l, double *acc) {
      if (S == W || l < S)
        for (I i = l; i < n_items; i += S) item(i, acc);
    }, out);
  }
};
#ifdef __HIPCC__
// device: a lane of the wave
template <int W>
struct LmWaveLanes {
  int lane;
  __device__ __forceinline__ bool lead() const { return lane == 0; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  template <int C, class F>
  __device__ __forceinline__ void sum(int n, F part, double *out) const {
    for (int c = 0; c < C; ++c) out[c] = 0.0;
    part(lane, out);
    for (int c = 0; c < n; ++c) out[c] = lm_group_sum<W>(out[c]);
  }
  template <int C, int S = W, class I, class F>
  __device__ __forceinline__ void over(I n_items, int n, F item, double *out) const {
    sum<C>(n, [&](int l, double *acc) {
      if (S == W || l < S)
        for (I i = l; i < n_items; i += S) item(i, acc);
    }, out);
  }
};
#endif

// ---- the chunked reduction of the coupled solves: two sums over any number of items in an order no
// grid decides.  A wave64 owns a chunk of 256 items -- lane stride, then the xor tree -- and writes chunk[ch] and
// chunk[stride + ch]; one wave then reduces the chunk results the same way.  item(i, &a, &b) adds item i's terms to the
// lane's two sums.  With stride 0 there is one sum: the second is not stored, and its total repeats the first ----
constexpr int kLmWave = 64, kLmChunk = 256;
constexpr int lm_chunks_of(long long n) { return n > 0 ? (int)((n + kLmChunk - 1) / kLmChunk) : 1; }

template <class F>
inline void lm_chunks_host(double *chunk, int n_items, int n_chunks, int stride, int nt, F item) {
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int ch = 0; ch < n_chunks; ++ch) {
    double part[kLmWave][2], out[2];
    const int base = ch * kLmChunk;
    for (int l = 0; l < kLmWave; ++l) {
      part[l][0] = part[l][1] = 0.0;
      for (int i = l; i < kLmChunk && base + i < n_items; i += kLmWave) item(base + i, &part[l][0], &part[l][1]);
    }
    lm_tree_host(part, 2, out);
    chunk[ch] = out[0];
    if (stride) chunk[stride + ch] = out[1];
  }
}
// the totals of the first n chunks
inline void lm_totals_host(const double *chunk, int n, int stride, double *a, double *b) {
  double part[kLmWave][2], out[2];
  for (int l = 0; l < kLmWave; ++l) {
    part[l][0] = part[l][1] = 0.0;
    for (int c = l; c < n; c += kLmWave) {
      part[l][0] = part[l][0] + chunk[c];
      part[l][1] = part[l][1] + chunk[stride + c];
    }
  }
  lm_tree_host(part, 2, out);
  *a = out[0];
  *b = out[1];
}
#ifdef __HIPCC__
// device: the chunk of workgroup blockIdx.x, one wave64; every lane returns both sums
template <class F>
__device__ __forceinline__ void lm_chunk_sums(int n_items, F item, double *a, double *b) {
  const int base = blockIdx.x * kLmChunk;
  double x = 0.0, y = 0.0;
  for (int i = threadIdx.x; i < kLmChunk && base + i < n_items; i += kLmWave) item(base + i, &x, &y);
  *a = lm_group_sum<kLmWave>(x);
  *b = lm_group_sum<kLmWave>(y);
}
// device: the totals of the first n chunks by one wave64
__device__ __forceinline__ void lm_totals(const double *chunk, int n, int stride, double *a, double *b) {
  double x = 0.0, y = 0.0;
  for (int c = threadIdx.x; c < n; c += kLmWave) {
    x = x + chunk[c];
    y = y + chunk[stride + c];
  }
  *a = lm_group_sum<kLmWave>(x);
  *b = lm_group_sum<kLmWave>(y);
}
// the workgroups a launch needs for n items, `per` each: one at least
inline unsigned lm_blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }
#endif

// ---- the pieces of a coupled linearisation ----
// one residual block added to the sums of NC unknowns: rho' J^T J (upper triangle by rows), then rho' J^T r, the
// products of the NR residuals paired as (j0 j0 + j1 j1) [+ j2 j2]
template <int NR, int NC>
LT_HD void lm_block_add(const double r[NR], double rho1, const double J[NR][NC], double acc[lm_sums(NC)]) {
  static_assert(NR == 2 || NR == 3, "two or three residuals");
  int o = 0;
  for (int x = 0; x < NC; ++x)
    for (int y = x; y < NC; ++y, ++o) {
      double s = J[0][x] * J[0][y] + J[1][x] * J[1][y];
      if (NR == 3) s = s + J[NR - 1][x] * J[NR - 1][y];
      acc[o] = acc[o] + rho1 * s;
    }
  for (int x = 0; x < NC; ++x, ++o) {
    double s = J[0][x] * r[0] + J[1][x] * r[1];
    if (NR == 3) s = s + J[NR - 1][x] * r[NR - 1];
    acc[o] = acc[o] + rho1 * s;
  }
}

// a block's term of the model decrease, rho' ((J d) . r + |J d|^2 / 2), from jd = J d
template <int NR>
LT_HD double lm_model_term(const double jd[NR], const double r[NR], double rho1) {
  static_assert(NR == 2 || NR == 3, "two or three residuals");
  double jr = jd[0] * r[0] + jd[1] * r[1], jj = jd[0] * jd[0] + jd[1] * jd[1];
  if (NR == 3) {
    jr = jr + jd[NR - 1] * r[NR - 1];
    jj = jj + jd[NR - 1] * jd[NR - 1];
  }
  return rho1 * (jr + 0.5 * jj);
}

// the inverse of a symmetric positive block with nd <= 4 unknowns by the Cholesky recurrence of lm_step, column by
// column.  A and M are 4 x 4 by rows; the lower triangle of A's leading nd x nd part is read, the leading nd x nd part
// of M is written.  false: a pivot is not positive or not finite (M is then as it was)
LT_HD bool lm_inverse4(const double *A, int nd, double *M) {
  double L[4][4];
  for (int i = 0; i < nd; ++i)
    for (int j = 0; j <= i; ++j) {
      double sum = A[4 * i + j];
      for (int k = 0; k < j; ++k) sum = sum - L[i][k] * L[j][k];
      if (i == j) {
        if (!lm_pivot_ok(sum)) return false;
        L[i][i] = sqrt(sum);
      } else {
        L[i][j] = sum / L[j][j];
      }
    }
  for (int c = 0; c < nd; ++c) {
    double y[4], x[4];
    for (int i = 0; i < nd; ++i) {
      double sum = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) sum = sum - L[i][k] * y[k];
      y[i] = sum / L[i][i];
    }
    for (int i = nd - 1; i >= 0; --i) {
      double sum = y[i];
      for (int k = i + 1; k < nd; ++k) sum = sum - L[k][i] * x[k];
      x[i] = sum / L[i][i];
    }
    for (int i = 0; i < nd; ++i) M[4 * i + c] = x[i];
  }
  return true;
}

// ---- geometry more than one minimiser evaluates ----
// CameraPose's constructor normalises its quaternion once (camera.h:94-95)
LT_HD void lm_normalise_q(const double q4[4], double q[4]) {
  const double n0 = sqrt((q4[0] * q4[0] + q4[2] * q4[2]) + (q4[1] * q4[1] + q4[3] * q4[3]));
  for (int i = 0; i < 4; ++i) q[i] = n0 > 0.0 ? q4[i] / n0 : q4[i];
}

// ceres::QuaternionRotatePoint: normalises, then UnitQuaternionRotatePoint in its cross-product form.  TP: the point's
// scalar -- a double where the point is a constant (it does not become a jet), TQ where it is a variable
template <class TQ, class TP>
LT_HD void lm_rotate(const TQ q[4], const TP p[3], TQ r[3]) {
  const TQ scale = 1.0 / rf_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const TQ a = scale * q[0], b = scale * q[1], c = scale * q[2], d = scale * q[3];
  TQ uv0 = c * p[2] - d * p[1], uv1 = d * p[0] - b * p[2], uv2 = b * p[1] - c * p[0];
  uv0 = uv0 + uv0; uv1 = uv1 + uv1; uv2 = uv2 + uv2;
  r[0] = p[0] + a * uv0; r[1] = p[1] + a * uv1; r[2] = p[2] + a * uv2;
  r[0] = r[0] + (c * uv2 - d * uv1);
  r[1] = r[1] + (d * uv0 - b * uv2);
  r[2] = r[2] + (b * uv1 - c * uv0);
}

// Line_WorldToPixel (line_projection.h:14-80) by its matrix products, the zero entries of the skew matrices and of K
// left out (they add an exact zero): R [m]x R^T - t (R d)^T + (R d) t^T, then K [m']x K^T and the normalisation of
// Line_ImgFromCam.  TV: the view's scalar -- a double for a constant camera, T where R and t carry derivatives
template <class T, class TV>
LT_HD void lm_w2p(const double k[4], const TV R[9], const TV t[3], const T d[3], const T m[3], T c[3]) {
  T Rd[3], RS[3][3];
  for (int i = 0; i < 3; ++i) {
    const TV r0 = R[3 * i], r1 = R[3 * i + 1], r2 = R[3 * i + 2];
    Rd[i] = (d[0] * r0 + d[1] * r1) + d[2] * r2;
    RS[i][0] = m[2] * r1 + (-m[1]) * r2;
    RS[i][1] = (-m[2]) * r0 + m[0] * r2;
    RS[i][2] = m[1] * r0 + (-m[0]) * r1;
  }
  // M(i, j) = ((R S R^T)(i, j) - t_i (R d)_j) + (R d)_i t_j at (2, 1), (0, 2), (1, 0)
  const int ii[3] = {2, 0, 1}, jj[3] = {1, 2, 0};
  T mt[3];
  for (int e = 0; e < 3; ++e) {
    const int i = ii[e], j = jj[e];
    const T rmr = (RS[i][0] * R[3 * j] + RS[i][1] * R[3 * j + 1]) + RS[i][2] * R[3 * j + 2];
    mt[e] = (rmr - Rd[j] * t[i]) + Rd[i] * t[j];
  }
  const double fx = k[0], fy = k[1], cx = k[2], cy = k[3];
  const T c0 = mt[0] * fy;
  const T c1 = mt[1] * fx;
  const T c2 = (mt[2] * fy + (-mt[1]) * cy) * fx + ((-mt[0]) * fy) * cx;
  const T cn = rf_sqrt(((c0 * c0 + c1 * c1) + c2 * c2) + kEps);
  c[0] = c0 / cn; c[1] = c1 / cn; c[2] = c2 / cn;
}

}  // namespace lt
