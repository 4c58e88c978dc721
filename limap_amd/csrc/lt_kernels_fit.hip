// lt_kernels_fit.hip -- limap's line fitter on the GPU: estimate_seg3d_from_depth (fitting/fitting.py:20-53) and
// Fit3DPoints (fitting/line3d_estimator.cc:7-109) with LO-MSAC (RansacLib's LocallyOptimizedMSAC as DESIGN §12
// restates it).
//
// One wave64 workgroup per segment (or point set).  The wave walks the problem's control flow in lockstep: every lane
// holds the same RANSAC state and draws the same random numbers, so every branch is uniform; the per-point work (the
// raster, the median ranks, the residual passes, the inlier lists) is lane-strided.  The points and two index lists
// live in LDS when the problem has at most kFitLds points, else in a slice of a global scratch buffer taken with one
// atomic (the same code through a generic pointer, so the same bits); a slice that does not fit marks the problem -1
// and the host runs the batch again with the counted size.
//
// Numerical contract (the CPU restatement under tests/ follows it to the bit):
//   MSAC score: lane l sums min(r2, t2) of points l, l + 64, ... from 0.0, lanes fold by xor 32, 16, ..., 1;
//   centroid and covariance: sequential in sample order; eigenvector: cyclic Jacobi (eig3_min);
//   generator: SplitMix64's finaliser keyed by (seed, image id, line, stream), draw c = fmix(key + (c + 1) GOLD) >> 32,
//   uniform(n) by rejection of draws below 2^32 mod n; stream 0 draws the minimal samples, stream 1 the shuffles.
#include "lt_devfn.h"
#include "lt_fit.h"

using namespace lt;

namespace {

constexpr unsigned long long kGold = 0x9E3779B97F4A7C15ull;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kLn2 = 0.6931471805599453;

__device__ __forceinline__ unsigned long long fmix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Rng {
  unsigned long long k, c;
  __device__ void init(unsigned long long seed, int img_id, long long line, unsigned long long stream) {
    k = fmix(seed + kGold);
    k = fmix(k ^ ((unsigned long long)(unsigned)img_id + kGold));
    k = fmix(k ^ ((unsigned long long)line + kGold));
    k = fmix(k ^ (stream + kGold));
    c = 0;
  }
  __device__ unsigned draw() {
    ++c;
    return (unsigned)(fmix(k + c * kGold) >> 32);
  }
  __device__ int uniform(int n) {  // n >= 1
    const unsigned un = (unsigned)n, thr = (0u - un) % un;
    for (;;) {
      const unsigned u = draw();
      if (u >= thr) return (int)(u % un);
    }
  }
};

struct Mdl {
  double d0, d1, d2, m0, m1, m2;
  int lo;  // made by the non-minimal solver
};

struct Store {
  double *x, *y, *z;
  int *la, *lb;
  int n;
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ double resid(const Mdl &M, double X, double Y, double Z) {
  // |q - proj|^2, proj = q + d x (m + d x q) (base/infinite_line.cc:55-59)
  const double c0 = M.d1 * Z - M.d2 * Y, c1 = M.d2 * X - M.d0 * Z, c2 = M.d0 * Y - M.d1 * X;
  const double q0 = M.m0 + c0, q1 = M.m1 + c1, q2 = M.m2 + c2;
  const double e0 = M.d1 * q2 - M.d2 * q1, e1 = M.d2 * q0 - M.d0 * q2, e2 = M.d0 * q1 - M.d1 * q0;
  const double f0 = X - (X + e0), f1 = Y - (Y + e1), f2 = Z - (Z + e2);
  return (f0 * f0 + f1 * f1) + f2 * f2;
}

__device__ double score(const Store &S, const Mdl &M, double t2) {
  double acc = 0.0;
  for (int k = lane_id(); k < S.n; k += 64) {
    const double r = resid(M, S.x[k], S.y[k], S.z[k]);
    acc += (t2 < r) ? t2 : r;  // std::min(r, t2)
  }
  return wave_sum(acc);
}

// GetInliers: indices with r2 < thr, in data order
__device__ int inliers(const Store &S, const Mdl &M, double thr, int *list) {
  int cnt = 0;
  for (int b = 0; b < S.n; b += 64) {
    const int k = b + lane_id();
    const bool in = k < S.n && resid(M, S.x[k], S.y[k], S.z[k]) < thr;
    const unsigned long long m = __ballot(in);
    if (in) list[cnt + __popcll(m & lanemask_lt())] = k;
    cnt += __popcll(m);
  }
  __syncthreads();
  return cnt;
}

__device__ int count_inliers(const Store &S, const Mdl &M, double thr) {
  int cnt = 0;
  for (int b = 0; b < S.n; b += 64) {
    const int k = b + lane_id();
    cnt += __popcll(__ballot(k < S.n && resid(M, S.x[k], S.y[k], S.z[k]) < thr));
  }
  return cnt;
}

// the project's 3x3 symmetric eigen-solver: cyclic Jacobi over (0,1), (0,2), (1,2), at most 16 sweeps; the eigenvector
// of the smallest eigenvalue (Eigen's col(0)), unit length, its largest-magnitude entry positive
__device__ bool eig3_min(const double C[6], double v[3]) {
  for (int i = 0; i < 6; ++i)
    if (!isfinite(C[i])) return false;
  double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, Rr[3] = {2, 1, 0};
  for (int sw = 0; sw < 16; ++sw) {
    const double off = (fabs(a[0][1]) + fabs(a[0][2])) + fabs(a[1][2]);
    if (off == 0.0) break;
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      const int p = P[pr], q = Q[pr], r = Rr[pr];
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
      if (theta < 0.0) t = -t;
      const double c = 1.0 / sqrt(t * t + 1.0);
      const double s = t * c;
      const double app = a[p][p] - t * apq, aqq = a[q][q] + t * apq;
      const double arp = a[r][p], arq = a[r][q];
      const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
      a[r][p] = a[p][r] = nrp;
      a[r][q] = a[q][r] = nrq;
      a[p][p] = app; a[q][q] = aqq;
      a[p][q] = a[q][p] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
      }
    }
  }
  int k = 0;
  if (a[1][1] < a[0][0]) k = 1;
  if (a[2][2] < (k == 0 ? a[0][0] : a[1][1])) k = 2;
  double w0 = k == 0 ? V[0][0] : (k == 1 ? V[0][1] : V[0][2]);
  double w1 = k == 0 ? V[1][0] : (k == 1 ? V[1][1] : V[1][2]);
  double w2 = k == 0 ? V[2][0] : (k == 1 ? V[2][1] : V[2][2]);
  const double nrm = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  w0 = w0 / nrm; w1 = w1 / nrm; w2 = w2 / nrm;
  int j = 0;
  double aj = fabs(w0);
  if (fabs(w1) > aj) { j = 1; aj = fabs(w1); }
  if (fabs(w2) > aj) j = 2;
  const double vj = j == 0 ? w0 : (j == 1 ? w1 : w2);
  if (vj < 0.0) { w0 = -w0; w1 = -w1; w2 = -w2; }
  v[0] = w0; v[1] = w1; v[2] = w2;
  return true;
}

// NonMinimalSolver (line3d_estimator.cc:71-101): centroid, covariance / (k - 1), smallest eigenvector
__device__ bool nonminimal(const Store &S, const int *smp, int k, Mdl &out) {
  if (k < 6) return false;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = 0; i < k; ++i) {
    const int id = smp[i];
    sx += S.x[id]; sy += S.y[id]; sz += S.z[id];
  }
  const double kd = (double)k;
  const double cx = sx / kd, cy = sy / kd, cz = sz / kd;
  double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < k; ++i) {
    const int id = smp[i];
    const double a = S.x[id] - cx, b = S.y[id] - cy, e = S.z[id] - cz;
    C[0] += a * a; C[1] += a * b; C[2] += a * e; C[3] += b * b; C[4] += b * e; C[5] += e * e;
  }
  const double den = (double)(k - 1);
  for (int i = 0; i < 6; ++i) C[i] = C[i] / den;
  double v[3];
  if (!eig3_min(C, v)) return false;
  out.d0 = v[0]; out.d1 = v[1]; out.d2 = v[2];
  out.m0 = cy * v[2] - cz * v[1];
  out.m1 = cz * v[0] - cx * v[2];
  out.m2 = cx * v[1] - cy * v[0];
  out.lo = 1;
  return true;
}

// MinimalSolver (line3d_estimator.cc:51-69)
__device__ bool minimal(const Store &S, int i0, int i1, Mdl &out) {
  const double p0 = S.x[i0], p1 = S.y[i0], p2 = S.z[i0];
  const double d0 = S.x[i1] - p0, d1 = S.y[i1] - p1, d2 = S.z[i1] - p2;
  const double ln = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  if (isnan(ln) || ln < 1e-12) return false;
  out.d0 = d0 / ln; out.d1 = d1 / ln; out.d2 = d2 / ln;
  out.m0 = p1 * out.d2 - p2 * out.d1;
  out.m1 = p2 * out.d0 - p0 * out.d2;
  out.m2 = p0 * out.d1 - p1 * out.d0;
  out.lo = 0;
  return true;
}

// utils::RandomShuffleAndResize: the first `target` steps of the Fisher-Yates shuffle (lane 0 swaps)
__device__ int shuffle_resize(int *list, int m, int target, Rng &rng) {
  if (m <= target) return m;
  for (int i = 0; i < target; ++i) {
    const int j = i + rng.uniform(m - i);
    if (lane_id() == 0) {
      const int t = list[i];
      list[i] = list[j];
      list[j] = t;
    }
  }
  __syncthreads();
  return target;
}

__device__ double lt_log(double x) {
  if (isnan(x) || x < 0.0) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (isinf(x)) return x;
  int e;
  double m = frexp(x, &e);
  if (m < 0.7071067811865476) { m = m * 2.0; e -= 1; }
  const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
  double p = 1.0 / 25.0;
  for (int k = 23; k >= 1; k -= 2) p = p * s2 + 1.0 / (double)k;
  return (double)e * kLn2 + 2.0 * (s * p);
}

__device__ int num_required(double ratio, double pmiss, int min_it, int max_it) {
  if (ratio <= 0.0) return max_it;
  if (ratio >= 1.0) return min_it;
  const double q = 1.0 - ratio * ratio;
  if (q >= 0.99999999999999) return max_it;
  const double it = ceil(lt_log(pmiss) / lt_log(q) + 0.5);
  const int n = it < (double)max_it ? (int)it : max_it;
  return n > min_it ? n : min_it;
}

struct Fit {
  Store S;
  FitCfg cfg;
  double t2;
  Rng smp, shf;

  __device__ void lsq_fit(double thr, Mdl &m) {  // LeastSquaresFit
    const int cnt = inliers(S, m, thr, S.lb);
    if (cnt < 2) return;
    const int k = shuffle_resize(S.lb, cnt, min(cfg.min_smp_mult * 2, cnt), shf);
    Mdl r;
    if (nonminimal(S, S.lb, k, r)) m = r;
  }

  __device__ void local_opt(Mdl &best, double &best_score) {  // LocalOptimization
    if (6 > S.n) return;
    const double mult = cfg.mult;
    Mdl m_init = best;
    lsq_fit(t2 * mult, m_init);
    double sc = score(S, m_init, t2);
    if (sc < best_score) { best_score = sc; best = m_init; }
    const int nb = inliers(S, m_init, t2 * mult, S.la);
    const int k_nm = max(6, min(2 * cfg.nonmin_mult, nb / 2));
    for (int r = 0; r < cfg.num_lo; ++r) {
      for (int k = lane_id(); k < nb; k += 64) S.lb[k] = S.la[k];
      __syncthreads();
      const int ks = shuffle_resize(S.lb, nb, k_nm, shf);
      Mdl mnm;
      if (!nonminimal(S, S.lb, ks, mnm)) continue;
      sc = score(S, mnm, t2);
      if (sc < best_score) { best_score = sc; best = mnm; }
      lsq_fit(t2, mnm);
      double thresh = mult * t2;
      const double upd = (mult - 1.0) * t2 / (double)(cfg.num_lsq - 1);
      for (int i = 0; i < cfg.num_lsq; ++i) {
        lsq_fit(thresh, mnm);
        sc = score(S, mnm, t2);
        if (sc < best_score) { best_score = sc; best = mnm; }
        thresh -= upd;
      }
    }
  }

  // LocallyOptimizedMSAC::EstimateModel; on return S.la holds the inliers of `best` (count returned)
  __device__ int run(Mdl &best, int &n_iter, int &n_lo, double &ratio) {
    const int n = S.n;
    best = Mdl{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
    n_iter = 0; n_lo = 0; ratio = 0.0;
    if (2 > n) return 0;
    double best_score = kDblMax, best_min_score = kDblMax;
    Mdl best_min = best;
    bool have = false;
    int max_it = max(cfg.max_it, cfg.min_it);
    int cnt = 0;
    int it = 0;
    for (; it < max_it; ++it) {
      if (it == cfg.lo_start && best_min_score < kDblMax) {
        ++n_lo;
        local_opt(best, best_score);
        cnt = count_inliers(S, best, t2);
        ratio = (double)cnt / (double)n;
        max_it = num_required(ratio, cfg.pmiss, cfg.min_it, cfg.max_it);
        have = true;
      }
      const int i0 = smp.uniform(n);
      int i1;
      do { i1 = smp.uniform(n); } while (i1 == i0);
      Mdl mdl;
      if (!minimal(S, i0, i1, mdl)) continue;
      const double sc = score(S, mdl, t2);
      const double loc = sc < kDblMax ? sc : kDblMax;
      if (loc < best_min_score || it == cfg.lo_start) {
        const bool k_best = loc < best_min_score;
        if (k_best) {
          best_min_score = loc;
          best_min = mdl;
          if (best_min_score < best_score) { best_score = best_min_score; best = best_min; }
        }
        const bool run_lo = it >= cfg.lo_start && best_min_score < kDblMax;
        if (!k_best && !run_lo) continue;
        if (run_lo) {
          ++n_lo;
          double s2 = best_min_score;
          local_opt(best_min, s2);
          if (s2 < best_score) { best_score = s2; best = best_min; }
        }
        cnt = count_inliers(S, best, t2);
        ratio = (double)cnt / (double)n;
        max_it = num_required(ratio, cfg.pmiss, cfg.min_it, cfg.max_it);
        have = true;
      }
    }
    n_iter = it;
    if (it <= cfg.lo_start && best_score < kDblMax) {
      ++n_lo;
      local_opt(best, best_score);
      cnt = count_inliers(S, best, t2);
      ratio = (double)cnt / (double)n;
      have = true;
    }
    if (cfg.final_ls) {
      const int k = have ? inliers(S, best, t2, S.la) : 0;
      Mdl refined = best;
      Mdl r;
      if (nonminimal(S, S.la, k, r)) refined = r;
      const double sc = score(S, refined, t2);
      if (sc < best_score) {
        best_score = sc;
        best = refined;
        cnt = count_inliers(S, best, t2);
        ratio = (double)cnt / (double)n;
        have = true;
      }
    }
    return have ? inliers(S, best, t2, S.la) : 0;
  }
};

// Fit3DPoints' segment (line3d_estimator.cc:28-43): extreme projections of the inliers from the first inlier
__device__ void endpoints(const Store &S, const Mdl &M, int cnt, double out[6]) {
  for (int k = 0; k < 6; ++k) out[k] = 0.0;
  if (cnt == 0) return;
  const int r = S.la[0];
  const double r0 = S.x[r], r1 = S.y[r], r2 = S.z[r];
  double lo = kDblMax, hi = -kDblMax;
  for (int k = lane_id(); k < cnt; k += 64) {
    const int id = S.la[k];
    const double p = ((S.x[id] - r0) * M.d0 + (S.y[id] - r1) * M.d1) + (S.z[id] - r2) * M.d2;
    lo = p < lo ? p : lo;
    hi = p > hi ? p : hi;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    const double a = __shfl_xor(lo, s, 64), b = __shfl_xor(hi, s, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  out[0] = r0 + M.d0 * lo; out[1] = r1 + M.d1 * lo; out[2] = r2 + M.d2 * lo;
  out[3] = r0 + M.d0 * hi; out[4] = r1 + M.d1 * hi; out[5] = r2 + M.d2 * hi;
}

// the store of a problem with up to `need` points: LDS, or a slice of the global scratch (nullptr: no room)
__device__ bool take_store(int need, double *s_x, double *s_y, double *s_z, int *s_a, int *s_b, double *scratch,
                           unsigned long long cap, unsigned long long *cnt, Store &S) {
  if (need <= kFitLds) {
    S.x = s_x; S.y = s_y; S.z = s_z; S.la = s_a; S.lb = s_b;
    return true;
  }
  unsigned long long base = 0;
  if (lane_id() == 0) base = atomicAdd(cnt, (unsigned long long)need);
  base = __shfl(base, 0, 64);
  if (base + (unsigned long long)need > cap) return false;
  double *p = scratch + 4ull * base;  // 32 B per point: x, y, z, two int lists
  S.x = p; S.y = p + need; S.z = p + 2 * (size_t)need;
  S.la = reinterpret_cast<int *>(p + 3 * (size_t)need);
  S.lb = S.la + need;
  return true;
}

// runs the fit, writes segment, status and stats; returns the inlier count (the list stays in F.S.la)
__device__ int finish(Fit &F, double *seg3d, int *status, int *stats, long long g, int kept) {
  Mdl best;
  int n_iter, n_lo;
  double ratio;
  const int cnt = F.run(best, n_iter, n_lo, ratio);
  double e[6];
  endpoints(F.S, best, cnt, e);
  const bool ok = !(ratio < F.cfg.min_pct);
  if (lane_id() == 0) {
    for (int k = 0; k < 6; ++k) seg3d[6 * g + k] = ok ? e[k] : 0.0;
    status[g] = ok ? 0 : 2;
    int *o = stats + 5 * g;
    o[0] = kept; o[1] = cnt; o[2] = n_iter; o[3] = n_lo; o[4] = (cnt > 0 && best.lo) ? 1 : 0;
  }
  return cnt;
}

__global__ __launch_bounds__(64) void k_fit_depth(int n_img, const FitImg *__restrict__ imgs,
                                                  const double *__restrict__ segs, const Cam *__restrict__ cams,
                                                  FitCfg cfg, double *scratch, unsigned long long scratch_cap,
                                                  unsigned long long *scratch_cnt, double *seg3d, int *status,
                                                  int *stats) {
  __shared__ double s_x[kFitLds], s_y[kFitLds], s_z[kFitLds];
  __shared__ int s_a[kFitLds], s_b[kFitLds];
  __shared__ double s_med[2];
  const long long g = blockIdx.x;
  // the image of segment g: the last one whose seg_begin <= g
  int lo = 0, hi = n_img - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (imgs[mid].seg_begin <= g) lo = mid; else hi = mid - 1;
  }
  const FitImg im = imgs[lo];
  const long long line = g - im.seg_begin;
  const Cam &cam = cams[im.cam];
  // seg2d.astype(int), Bresenham by the sign / major-axis rule (ties y-major); only the indices whose major coordinate
  // lies inside the image are walked, the minor coordinate is filtered per pixel
  const long long x0 = (long long)segs[4 * g], y0 = (long long)segs[4 * g + 1];
  const long long x1 = (long long)segs[4 * g + 2], y1 = (long long)segs[4 * g + 3];
  const long long dx = x1 - x0, dy = y1 - y0;
  const long long xs = dx > 0 ? 1 : -1, ys = dy > 0 ? 1 : -1;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const bool xmaj = adx > ady;
  const long long a0 = xmaj ? x0 : y0, sa = xmaj ? xs : ys, A = xmaj ? im.w : im.h;
  const long long m0 = xmaj ? y0 : x0, sm = xmaj ? ys : xs, Mx = xmaj ? im.h : im.w;
  const long long dmaj = xmaj ? adx : ady, dmin = xmaj ? ady : adx;
  long long ilo, ihi;
  if (sa > 0) { ilo = max(0ll, -a0); ihi = min(dmaj, A - 1 - a0); }
  else { ilo = max(0ll, a0 - A + 1); ihi = min(dmaj, a0); }
  const int need = ihi >= ilo ? (int)(ihi - ilo + 1) : 0;
  Store S;
  if (!take_store(need, s_x, s_y, s_z, s_a, s_b, scratch, scratch_cap, scratch_cnt, S)) {
    if (lane_id() == 0) status[g] = -1;
    return;
  }
  const char *base = reinterpret_cast<const char *>(im.map);
  int n = 0;
  bool any_nan = false;
  for (long long b = ilo; b <= ihi; b += 64) {
    const long long i = b + lane_id();
    bool keep = false;
    double px = 0.0, py = 0.0, dv = 0.0;
    if (i <= ihi) {
      const long long k = dmaj > 0 ? (2 * dmin * i + dmaj) / (2 * dmaj) : 0;
      const long long a = a0 + sa * i, m = m0 + sm * k;
      if (m >= 0 && m < Mx) {
        const long long X = xmaj ? a : m, Y = xmaj ? m : a;
        const long long at = Y * im.stride + X;
        dv = im.dtype == 0 ? (double)reinterpret_cast<const float *>(base)[at]
                           : reinterpret_cast<const double *>(base)[at];
        keep = !isinf(dv);
        px = (double)X; py = (double)Y;
      }
    }
    const unsigned long long mk = __ballot(keep);
    if (keep) {
      const int pos = n + __popcll(mk & lanemask_lt());
      S.x[pos] = px; S.y[pos] = py; S.z[pos] = dv;
    }
    any_nan = any_nan || __ballot(keep && isnan(dv)) != 0ull;
    n += __popcll(mk);
  }
  __syncthreads();
  S.n = n;
  if (n <= 6) {
    if (lane_id() == 0) {
      for (int k = 0; k < 6; ++k) seg3d[6 * g + k] = 0.0;
      status[g] = 1;
      int *o = stats + 5 * g;
      o[0] = n; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0;
    }
    return;
  }
  // exact median: the element of stable rank (n-1)/2 and n/2 (ranks count smaller values, then equal ones before it)
  const int k1 = (n - 1) / 2, k2 = n / 2;
  for (int i = lane_id(); i < n; i += 64) {
    const double v = S.z[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double w = S.z[j];
      rank += (w < v || (w == v && j < i)) ? 1 : 0;
    }
    if (rank == k1) s_med[0] = v;
    if (rank == k2) s_med[1] = v;
  }
  __syncthreads();
  double unc;
  if (im.dtype == 0) {  // np.median of float32 stays float32; var2d * median is rounded to float32
    float med = any_nan ? __builtin_nanf("") : (float)s_med[0];
    if (!any_nan && (n % 2) == 0) med = ((float)s_med[0] + (float)s_med[1]) / 2.0f;
    const float u = (float)cfg.var2d * med;
    unc = (double)u / cam.f;
  } else {
    double med = any_nan ? __builtin_nan("") : s_med[0];
    if (!any_nan && (n % 2) == 0) med = (s_med[0] + s_med[1]) / 2.0;
    unc = (cfg.var2d * med) / cam.f;
  }
  const double th = cfg.ransac_th * unc;
  // unproject: ((x - cx) / fx, (y - cy) / fy, 1) * depth, then R^T p - R^T t
  const double *R = cam.R;
  const double ct0 = (R[0] * cam.t[0] + R[3] * cam.t[1]) + R[6] * cam.t[2];
  const double ct1 = (R[1] * cam.t[0] + R[4] * cam.t[1]) + R[7] * cam.t[2];
  const double ct2 = (R[2] * cam.t[0] + R[5] * cam.t[1]) + R[8] * cam.t[2];
  for (int k = lane_id(); k < n; k += 64) {
    const double d = S.z[k];
    const double p0 = ((S.x[k] - cam.cx) / cam.fx) * d, p1 = ((S.y[k] - cam.cy) / cam.fy) * d, p2 = d;
    S.x[k] = ((R[0] * p0 + R[3] * p1) + R[6] * p2) - ct0;
    S.y[k] = ((R[1] * p0 + R[4] * p1) + R[7] * p2) - ct1;
    S.z[k] = ((R[2] * p0 + R[5] * p1) + R[8] * p2) - ct2;
  }
  __syncthreads();
  Fit F;
  F.S = S;
  F.cfg = cfg;
  F.t2 = th * th;
  F.smp.init(cfg.seed, im.img_id, line, 0);
  F.shf.init(cfg.seed, im.img_id, line, 1);
  finish(F, seg3d, status, stats, g, n);
}

__global__ __launch_bounds__(64) void k_fit_points(const long long *__restrict__ off, const double *__restrict__ xyz,
                                                   FitCfg cfg, double *scratch, unsigned long long scratch_cap,
                                                   unsigned long long *scratch_cnt, double *seg3d, int *status,
                                                   int *stats, unsigned char *mask) {
  __shared__ double s_x[kFitLds], s_y[kFitLds], s_z[kFitLds];
  __shared__ int s_a[kFitLds], s_b[kFitLds];
  const long long g = blockIdx.x;
  const long long p0 = off[g];
  const int n = (int)(off[g + 1] - p0);
  Store S;
  if (!take_store(n, s_x, s_y, s_z, s_a, s_b, scratch, scratch_cap, scratch_cnt, S)) {
    if (lane_id() == 0) status[g] = -1;
    return;
  }
  for (int k = lane_id(); k < n; k += 64) {
    S.x[k] = xyz[3 * (p0 + k)]; S.y[k] = xyz[3 * (p0 + k) + 1]; S.z[k] = xyz[3 * (p0 + k) + 2];
  }
  __syncthreads();
  S.n = n;
  Fit F;
  F.S = S;
  F.cfg = cfg;
  F.t2 = cfg.t2_points;
  F.smp.init(cfg.seed, -1, g, 0);
  F.shf.init(cfg.seed, -1, g, 1);
  const int cnt = finish(F, seg3d, status, stats, g, n);
  if (mask)  // stats.inlier_indices; the host zero-fills the mask
    for (int k = lane_id(); k < cnt; k += 64) mask[p0 + S.la[k]] = 1;
}


// ---- estimate_seg3d_from_points3d (fitting/fitting.py:56-102) -------------------------------------------------------
// the store of a scan problem: the points, the two index lists and the ray depths (40 B a point; the scratch counts
// 32-B units, so a slice takes need + ceil(need / 4) of them)
__device__ bool take_scan_store(int need, double *s_x, double *s_y, double *s_z, int *s_a, int *s_b, double *s_r,
                                double *scratch, unsigned long long cap, unsigned long long *cnt, Store &S, double *&rd) {
  if (need <= kFitLds) {
    S.x = s_x; S.y = s_y; S.z = s_z; S.la = s_a; S.lb = s_b;
    rd = s_r;
    return true;
  }
  const unsigned long long units = (unsigned long long)need + (unsigned long long)((need + 3) / 4);
  unsigned long long base = 0;
  if (lane_id() == 0) base = atomicAdd(cnt, units);
  base = __shfl(base, 0, 64);
  if (base + units > cap) return false;
  double *p = scratch + 4ull * base;
  S.x = p; S.y = p + need; S.z = p + 2 * (size_t)need;
  rd = p + 3 * (size_t)need;
  S.la = reinterpret_cast<int *>(p + 4 * (size_t)need);
  S.lb = S.la + need;
  return true;
}

// one corner of the scan: the three channels widened to double, 0 outside (grid_sample's zero padding)
__device__ __forceinline__ void scan_px(const ScanImg &im, long long ix, long long iy, double v[3]) {
  if (ix < 0 || iy < 0 || ix >= im.w || iy >= im.h) {
    v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
    return;
  }
  const long long at = iy * im.rs + ix * im.ps;
  if (im.dtype == 0) {
    const float *b = reinterpret_cast<const float *>(im.map) + at;
    v[0] = (double)b[0]; v[1] = (double)b[im.cs]; v[2] = (double)b[2 * im.cs];
  } else {
    const double *b = reinterpret_cast<const double *>(im.map) + at;
    v[0] = b[0]; v[1] = b[im.cs]; v[2] = b[2 * im.cs];
  }
}

// the index range [lo, hi] of np.linspace(start, stop, num) samples that can lie inside 0 < c < lim for both
// coordinates: the exact per-sample filter follows, so the range only has to be conservative (the sample error, a few
// ulps of |start| + |delta|, is covered 1000 times over by the margin in index units)
__device__ void scan_walk(const double s[4], long long num, double lim_x, double lim_y, long long &lo, long long &hi) {
  lo = 0; hi = num - 1;
  if (num <= 1) return;
  const double div = (double)(num - 1);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double s0 = s[c], d = s[2 + c] - s[c], lim = c == 0 ? lim_x : lim_y;
    const double step = d / div;
    if (d == 0.0) {
      if (!(0.0 < s0 && s0 < lim)) { lo = 1; hi = 0; }
      continue;
    }
    if (step == 0.0) continue;
    const double ta = (0.0 - s0) / step, tb = (lim - s0) / step;
    const double m = 2.0 + 1e-12 * ((fabs(s0) + fabs(d)) + lim) / fabs(step);
    const double a = (ta < tb ? ta : tb) - m, b = (ta < tb ? tb : ta) + m;
    if (a > (double)lo) lo = (long long)ceil(a);
    if (b < (double)hi) hi = (long long)floor(b);
  }
}

__global__ __launch_bounds__(64) void k_fit_scan(int n_img, const ScanImg *__restrict__ imgs,
                                                 const double *__restrict__ segs, const Cam *__restrict__ cams,
                                                 FitCfg cfg, double *scratch, unsigned long long scratch_cap,
                                                 unsigned long long *scratch_cnt, double *seg3d, int *status,
                                                 int *stats) {
  __shared__ double s_x[kFitLds], s_y[kFitLds], s_z[kFitLds], s_r[kFitLds];
  __shared__ int s_a[kFitLds], s_b[kFitLds];
  __shared__ double s_med[2];
  const long long g = blockIdx.x;
  int lo = 0, hi = n_img - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (imgs[mid].seg_begin <= g) lo = mid; else hi = mid - 1;
  }
  const ScanImg im = imgs[lo];
  const long long line = g - im.seg_begin;
  const Cam &cam = cams[im.cam];
  // num = int(norm(stop - start) * 2), the norm as sqrt(fma(dy, dy, dx * dx)); linspace as NumPy 2.2 evaluates it
  const double s[4] = {segs[4 * g], segs[4 * g + 1], segs[4 * g + 2], segs[4 * g + 3]};
  const double dx = s[2] - s[0], dy = s[3] - s[1];
  const long long num = (long long)(sqrt(fma(dy, dy, dx * dx)) * 2.0);
  const double div = (double)(num - 1);
  const double stx = dx / div, sty = dy / div;
  const bool step0 = stx == 0.0 || sty == 0.0;
  const double lim_x = (double)(im.img_w - 1), lim_y = (double)(im.img_h - 1);
  const double sw1 = (double)(im.w - 1), sh1 = (double)(im.h - 1);
  long long ilo, ihi;
  scan_walk(s, num, lim_x, lim_y, ilo, ihi);
  const int need = ihi >= ilo ? (int)(ihi - ilo + 1) : 0;
  Store S;
  double *rd;
  if (!take_scan_store(need, s_x, s_y, s_z, s_a, s_b, s_r, scratch, scratch_cap, scratch_cnt, S, rd)) {
    if (lane_id() == 0) status[g] = -1;
    return;
  }
  int n = 0;
  bool oor = false;
  for (long long b = ilo; b <= ihi; b += 64) {
    const long long i = b + lane_id();
    bool keep = false, bad = false;
    double v[3] = {0.0, 0.0, 0.0};
    if (i <= ihi) {
      double px, py;
      if (num == 1) { px = 0.0 * dx + s[0]; py = 0.0 * dy + s[1]; }
      else if (i == num - 1) { px = s[2]; py = s[3]; }
      else if (step0) { px = ((double)i / div) * dx + s[0]; py = ((double)i / div) * dy + s[1]; }
      else { px = (double)i * stx + s[0]; py = (double)i * sty + s[1]; }
      if (0.0 < px && 0.0 < py && px < lim_x && py < lim_y) {
        // interpolate_scan: kp / [W-1, H-1] * 2 - 1 (the scan's W, H), its (-1, 1) assert, then grid_sample with
        // align_corners: the coordinate goes through the normalise / unnormalise round trip
        const double gx = (px / sw1) * 2.0 - 1.0, gy = (py / sh1) * 2.0 - 1.0;
        if (gx > -1.0 && gx < 1.0 && gy > -1.0 && gy < 1.0) {
          const double ux = ((gx + 1.0) / 2.0) * sw1, uy = ((gy + 1.0) / 2.0) * sh1;
          const double fx0 = floor(ux), fy0 = floor(uy);
          const double wx = ux - fx0, wy = uy - fy0;
          const double ex = 1.0 - wx, ey = 1.0 - wy;
          const double nw = ey * ex, ne = ey * wx, sw = wy * ex, se = wy * wx;
          const long long x0 = (long long)fx0, y0 = (long long)fy0;
          double a[3], bb[3], c[3], d[3];
          scan_px(im, x0, y0, a); scan_px(im, x0 + 1, y0, bb);
          scan_px(im, x0, y0 + 1, c); scan_px(im, x0 + 1, y0 + 1, d);
          bool any = false;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            v[k] = fma(d[k], se, fma(c[k], sw, fma(bb[k], ne, a[k] * nw)));
            any = any || isnan(v[k]);
          }
          if (any) {  // mode="nearest" (round half to even) for the channels bilinear left NaN
            double nn[3];
            scan_px(im, (long long)rint(ux), (long long)rint(uy), nn);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = isnan(v[k]) ? nn[k] : v[k];
          }
          keep = !isnan(v[0]) && !isnan(v[1]) && !isnan(v[2]);
        } else {
          bad = true;
        }
      }
    }
    oor = oor || __ballot(bad) != 0ull;
    const unsigned long long mk = __ballot(keep);
    if (keep) {
      const int pos = n + __popcll(mk & lanemask_lt());
      S.x[pos] = v[0]; S.y[pos] = v[1]; S.z[pos] = v[2];
      rd[pos] = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    }
    n += __popcll(mk);
  }
  __syncthreads();
  S.n = n;
  if (oor || n <= 6) {
    if (lane_id() == 0) {
      for (int k = 0; k < 6; ++k) seg3d[6 * g + k] = 0.0;
      status[g] = oor ? 3 : 1;
      int *o = stats + 5 * g;
      o[0] = oor ? 0 : n; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0;
    }
    return;
  }
  // the exact median of the ray depths (no NaN: a kept sample has three non-NaN channels)
  const int k1 = (n - 1) / 2, k2 = n / 2;
  for (int i = lane_id(); i < n; i += 64) {
    const double v = rd[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double w = rd[j];
      rank += (w < v || (w == v && j < i)) ? 1 : 0;
    }
    if (rank == k1) s_med[0] = v;
    if (rank == k2) s_med[1] = v;
  }
  __syncthreads();
  const double med = (n % 2) == 0 ? (s_med[0] + s_med[1]) / 2.0 : s_med[0];
  const double unc = (cfg.var2d * med) / (0.7 * (double)(im.img_h > im.img_w ? im.img_h : im.img_w));
  const double th = cfg.ransac_th * unc;
  if (im.use_pose) {  // Tr[:3, :3] @ p + Tr[:3, 3]
    const double *T = im.pose;
    for (int k = lane_id(); k < n; k += 64) {
      const double X = S.x[k], Y = S.y[k], Z = S.z[k];
      S.x[k] = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
      S.y[k] = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
      S.z[k] = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    }
  } else {  // R^T p - R^T t
    const double *R = cam.R;
    const double ct0 = (R[0] * cam.t[0] + R[3] * cam.t[1]) + R[6] * cam.t[2];
    const double ct1 = (R[1] * cam.t[0] + R[4] * cam.t[1]) + R[7] * cam.t[2];
    const double ct2 = (R[2] * cam.t[0] + R[5] * cam.t[1]) + R[8] * cam.t[2];
    for (int k = lane_id(); k < n; k += 64) {
      const double X = S.x[k], Y = S.y[k], Z = S.z[k];
      S.x[k] = ((R[0] * X + R[3] * Y) + R[6] * Z) - ct0;
      S.y[k] = ((R[1] * X + R[4] * Y) + R[7] * Z) - ct1;
      S.z[k] = ((R[2] * X + R[5] * Y) + R[8] * Z) - ct2;
    }
  }
  __syncthreads();
  Fit F;
  F.S = S;
  F.cfg = cfg;
  F.t2 = th * th;
  F.smp.init(cfg.seed, im.img_id, line, 0);
  F.shf.init(cfg.seed, im.img_id, line, 1);
  finish(F, seg3d, status, stats, g, n);
}

}  // namespace

namespace lt {
void launch_fit_depth(hipStream_t st, long long n_segs, int n_img, const FitImg *imgs, const double *segs,
                      const Cam *cams, const FitCfg &cfg, double *scratch, unsigned long long scratch_cap,
                      unsigned long long *scratch_cnt, double *seg3d, int *status, int *stats) {
  if (n_segs <= 0) return;
  hipLaunchKernelGGL(k_fit_depth, dim3((unsigned)n_segs), dim3(64), 0, st, n_img, imgs, segs, cams, cfg, scratch,
                     scratch_cap, scratch_cnt, seg3d, status, stats);
}
void launch_fit_points(hipStream_t st, long long n_sets, const long long *off, const double *xyz, const FitCfg &cfg,
                       double *scratch, unsigned long long scratch_cap, unsigned long long *scratch_cnt, double *seg3d,
                       int *status, int *stats, unsigned char *mask) {
  if (n_sets <= 0) return;
  hipLaunchKernelGGL(k_fit_points, dim3((unsigned)n_sets), dim3(64), 0, st, off, xyz, cfg, scratch, scratch_cap,
                     scratch_cnt, seg3d, status, stats, mask);
}
void launch_fit_scan(hipStream_t st, long long n_segs, int n_img, const ScanImg *imgs, const double *segs,
                     const Cam *cams, const FitCfg &cfg, double *scratch, unsigned long long scratch_cap,
                     unsigned long long *scratch_cnt, double *seg3d, int *status, int *stats) {
  if (n_segs <= 0) return;
  hipLaunchKernelGGL(k_fit_scan, dim3((unsigned)n_segs), dim3(64), 0, st, n_img, imgs, segs, cams, cfg, scratch,
                     scratch_cap, scratch_cnt, seg3d, status, stats);
}
}  // namespace lt
