// lt_kernels_vp.hip -- device side of the vanishing-point detector (limap.vplib JLinkage).  A whole scene
// per set of launches: per-image offsets (VpImg) and a block table (VpBlock), as lt_kernels_bpt.hip does it.
//   k_vp_prep     per line: Line2d::length() and the `length() < min_length` filter (JLinkage.cc:19-23)
//   k_vp_lines    per valid line: endpoints rounded to FP32, midpoint, homogeneous coordinates
//   k_vp_hyp      hypothesis m of an image: the cross product of two valid lines drawn by the counter-based generator
//   k_vp_pref     the preference sets: a tile of hypotheses in LDS, one lane = one line x 64 hypotheses = one word
//   k_vp_cluster  J-Linkage: one workgroup per image merges the pair with the greatest Jaccard ratio until no two
//                 preference sets intersect
// FP64 and integers only, -ffp-contract=off; nothing here depends on the order in which lanes or workgroups run.

#include "lt_vp.h"

#include <climits>

namespace lt {

namespace {

__global__ void __launch_bounds__(kVpBlock) k_vp_prep(const double *__restrict__ lines4, long long n, double min_length,
                                                      unsigned char *__restrict__ flag) {
  const long long k = (long long)blockIdx.x * kVpBlock + threadIdx.x;
  if (k >= n) return;
  const double len = vp_length(lines4[4 * k], lines4[4 * k + 1], lines4[4 * k + 2], lines4[4 * k + 3]);
  flag[k] = len < min_length ? 0 : 1;
}

__global__ void __launch_bounds__(kVpBlock) k_vp_lines(const double *__restrict__ lines4,
                                                       const long long *__restrict__ src, long long n,
                                                       VpLine *__restrict__ out) {
  const long long s = (long long)blockIdx.x * kVpBlock + threadIdx.x;
  if (s >= n) return;
  const long long k = src[s];
  out[s] = vp_line(lines4[4 * k], lines4[4 * k + 1], lines4[4 * k + 2], lines4[4 * k + 3]);
}

// grid: images x ceil(n_hyp / kVpBlock) workgroups in x, an image's workgroups next to each other
__global__ void __launch_bounds__(kVpBlock) k_vp_hyp(const VpImg *__restrict__ imgs, int n_hyp, int blocks_per_img,
                                                     unsigned long long seed, const VpLine *__restrict__ lines,
                                                     VpHyp *__restrict__ hyp) {
  const VpImg im = imgs[blockIdx.x / (unsigned)blocks_per_img];
  const int m = (int)(blockIdx.x % (unsigned)blocks_per_img) * kVpBlock + (int)threadIdx.x;
  if (m >= n_hyp || im.n < 2) return;
  unsigned a, b;
  vp_sample(seed, (unsigned long long)m, (unsigned)im.n, &a, &b);
  hyp[im.h0 + m] = vp_hypothesis(lines[im.v0 + a], lines[im.v0 + b]);
}

__global__ void __launch_bounds__(kVpBlock) k_vp_pref(const VpBlock *__restrict__ blk, const VpImg *__restrict__ imgs,
                                                      int n_hyp, int n_words, double th,
                                                      const VpLine *__restrict__ lines, const VpHyp *__restrict__ hyp,
                                                      unsigned long long *__restrict__ pref) {
  __shared__ VpHyp s_hyp[kVpHypTile];
  const VpBlock b = blk[blockIdx.x];
  const VpImg im = imgs[b.img];
  const int m0 = b.w0 * 64;
  const int tile = n_hyp - m0 < kVpHypTile ? n_hyp - m0 : kVpHypTile;  // > 0: the host makes no empty block
  for (int t = threadIdx.x; t < tile; t += kVpBlock) s_hyp[t] = hyp[im.h0 + m0 + t];
  __syncthreads();
  const int k = b.k0 + (int)threadIdx.x;
  if (k >= im.n) return;
  const VpLine l = lines[im.v0 + k];
  for (int w = 0; w < kVpPrefWords && b.w0 + w < n_words; ++w) {
    unsigned long long word = 0ull;
    const int t1 = tile - 64 * w < 64 ? tile - 64 * w : 64;  // the padding bits stay zero
    for (int t = 0; t < t1; ++t)
      if (vp_inlier(l.x1, l.y1, l.cx, l.cy, s_hyp[64 * w + t], th)) word |= 1ull << t;
    pref[im.p0 + (long long)(b.w0 + w) * im.n + k] = word;
  }
}

// ---- clustering ----------------------------------------------------------------------------------------------------
struct Best {
  int c, u, i, j;  // intersection, union, the pair; none: (0, 1, INT_MAX, INT_MAX)
};
__device__ __forceinline__ Best best_none() { return Best{0, 1, INT_MAX, INT_MAX}; }
__device__ __forceinline__ Best best_of(Best a, Best b) {
  return vp_better(b.c, b.u, b.i, b.j, a.c, a.u, a.i, a.j) ? b : a;
}
__device__ __forceinline__ Best wave_best(Best v) {
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.c = __shfl_xor(v.c, off, 64);
    o.u = __shfl_xor(v.u, off, 64);
    o.i = __shfl_xor(v.i, off, 64);
    o.j = __shfl_xor(v.j, off, 64);
    v = best_of(v, o);
  }
  return v;
}
// every lane of the workgroup receives the best of all lanes' v (two barriers)
__device__ __forceinline__ Best block_best(Best v, Best *s_red) {
  constexpr int kWaves = kVpClBlock / 64;
  v = wave_best(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  Best r = s_red[0];
  for (int k = 1; k < kWaves; ++k) r = best_of(r, s_red[k]);
  return r;
}

__device__ __forceinline__ int inter_count(const unsigned long long *P, int n, int n_words, int a, int b) {
  int c = 0;
  for (int w = 0; w < n_words; ++w) c += __popcll(P[(long long)w * n + a] & P[(long long)w * n + b]);
  return c;
}

// the best partner k > row of cluster row, by one wave
__device__ __forceinline__ void scan_row(const unsigned long long *P, int n, int n_words, int row, int *psize, int *nn,
                                         int *ni, int *nu) {
  const int lane = threadIdx.x & 63;
  Best v = best_none();
  const int sz = psize[row];
  if (sz > 0)  // an empty preference set intersects nothing
    for (int k = row + 1 + lane; k < n; k += 64) {
      const int sk = psize[k];
      if (sk <= 0) continue;
      const int c = inter_count(P, n, n_words, row, k);
      if (c > 0) v = best_of(v, Best{c, sz + sk - c, row, k});
    }
  v = wave_best(v);
  if (lane == 0) {
    nn[row] = v.c > 0 ? v.j : -1;
    ni[row] = v.c;
    nu[row] = v.u;
  }
}

__global__ void __launch_bounds__(kVpClBlock) k_vp_cluster(const VpImg *__restrict__ imgs, int n_words,
                                                           unsigned long long *pref, int *g_state,
                                                           int *__restrict__ roots) {
  __shared__ int s_state[kVpStateInts * kVpLdsClusters];
  __shared__ Best s_red[kVpClBlock / 64];
  constexpr int kWaves = kVpClBlock / 64;
  const VpImg im = imgs[blockIdx.x];
  const int n = im.n;
  if (n <= 0) return;
  unsigned long long *P = pref + im.p0;
  int *state = n <= kVpLdsClusters ? s_state : g_state + kVpStateInts * im.v0;
  int *psize = state, *nn = state + n, *ni = state + 2 * n, *nu = state + 3 * n, *parent = state + 4 * n;
  const int tid = threadIdx.x, wave = tid >> 6;

  for (int k = tid; k < n; k += kVpClBlock) {
    int c = 0;
    for (int w = 0; w < n_words; ++w) c += __popcll(P[(long long)w * n + k]);
    psize[k] = c;
    parent[k] = -1;
  }
  __syncthreads();
  for (int row = wave; row < n; row += kWaves) scan_row(P, n, n_words, row, psize, nn, ni, nu);
  __syncthreads();

  for (int step = 0; step < n; ++step) {  // at most n - 1 merges
    Best v = best_none();
    for (int k = tid; k < n; k += kVpClBlock)
      if (psize[k] > 0 && nn[k] >= 0) v = best_of(v, Best{ni[k], nu[k], k, nn[k]});
    v = block_best(v, s_red);
    if (v.c <= 0) break;  // no two sets intersect (uniform: every lane holds the same v)
    const int i = v.i, j = v.j;
    // P_i <- P_i & P_j, |P_i| = the recorded intersection; j goes
    for (int w = tid; w < n_words; w += kVpClBlock) P[(long long)w * n + i] &= P[(long long)w * n + j];
    if (tid == 0) {
      psize[i] = v.c;
      psize[j] = -1;
      parent[j] = i;
    }
    __syncthreads();
    // the merged set against every live cluster: rows k < i compare their partner with the new (k, i); rows whose
    // partner was i or j are scanned again; the clusters k > i are row i's candidates
    Best mine = best_none();
    const int si = v.c;
    for (int k = tid; k < n; k += kVpClBlock) {
      const int sk = psize[k];
      if (sk < 0 || k == i) continue;
      const int p = nn[k];
      const bool again = k < j && (p == i || p == j);
      if (again) nn[k] = -2;
      if (sk == 0 || (again && k < i)) continue;
      const int c = inter_count(P, n, n_words, i, k);
      if (c <= 0) continue;
      const int u = si + sk - c;
      if (k < i) {
        if (p < 0 || vp_better(c, u, k, i, ni[k], nu[k], k, p)) {
          nn[k] = i;
          ni[k] = c;
          nu[k] = u;
        }
      } else {
        mine = best_of(mine, Best{c, u, i, k});
      }
    }
    mine = block_best(mine, s_red);
    if (tid == 0) {
      nn[i] = mine.c > 0 ? mine.j : -1;
      ni[i] = mine.c;
      nu[i] = mine.u;
    }
    __syncthreads();
    for (int row = wave; row < n; row += kWaves)
      if (psize[row] >= 0 && nn[row] == -2) scan_row(P, n, n_words, row, psize, nn, ni, nu);
    __syncthreads();
  }
  for (int k = tid; k < n; k += kVpClBlock) {
    int r = k;
    while (parent[r] >= 0) r = parent[r];
    roots[im.v0 + k] = r;
  }
}

inline int grid_of(long long n) { return (int)((n + kVpBlock - 1) / kVpBlock); }

}  // namespace

void launch_vp_prep(hipStream_t st, const double *lines4, long long n_lines, double min_length, unsigned char *flag) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_vp_prep, dim3(grid_of(n_lines)), dim3(kVpBlock), 0, st, lines4, n_lines, min_length, flag);
}

void launch_vp_lines(hipStream_t st, const double *lines4, const long long *src, long long n_valid, VpLine *out) {
  if (n_valid <= 0) return;
  hipLaunchKernelGGL(k_vp_lines, dim3(grid_of(n_valid)), dim3(kVpBlock), 0, st, lines4, src, n_valid, out);
}

void launch_vp_hyp(hipStream_t st, const VpImg *imgs, int n_act, int n_hyp, unsigned long long seed, const VpLine *lines,
                   VpHyp *hyp) {
  if (n_act <= 0 || n_hyp <= 0) return;
  const int per_img = grid_of(n_hyp);  // the caller keeps n_act * per_img within a launch (vp_launch_fits)
  hipLaunchKernelGGL(k_vp_hyp, dim3((unsigned)((long long)n_act * per_img)), dim3(kVpBlock), 0, st, imgs, n_hyp, per_img,
                     seed, lines, hyp);
}

void launch_vp_pref(hipStream_t st, const VpBlock *blk, int n_blk, const VpImg *imgs, int n_hyp, int n_words, double th,
                    const VpLine *lines, const VpHyp *hyp, unsigned long long *pref) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(k_vp_pref, dim3(n_blk), dim3(kVpBlock), 0, st, blk, imgs, n_hyp, n_words, th, lines, hyp, pref);
}

void launch_vp_cluster(hipStream_t st, const VpImg *imgs, int n_act, int n_words, unsigned long long *pref, int *state,
                       int *roots) {
  if (n_act <= 0) return;
  hipLaunchKernelGGL(k_vp_cluster, dim3(n_act), dim3(kVpClBlock), 0, st, imgs, n_words, pref, state, roots);
}

}  // namespace lt
