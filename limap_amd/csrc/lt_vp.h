// lt_vp.h -- records and the FP64 expressions shared by the host side (lt_vp.cpp) and the device side
// (lt_kernels_vp.hip) of the vanishing-point detector (limap.vplib: JLinkage, vplib/JLinkage/JLinkage.cc).  The
// hypothesis generator, the consistency test and the order of the clustering are this project's own definition
// (DESIGN §18); both sides compile the same inline functions with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

namespace lt {

constexpr int kVpBlock = 256;          // lanes per workgroup of k_vp_prep / k_vp_lines / k_vp_hyp / k_vp_pref
constexpr int kVpPrefWords = 8;        // 64-bit words of the preference set one k_vp_pref workgroup fills per line
constexpr int kVpHypTile = 64 * kVpPrefWords;  // hypotheses staged in LDS by k_vp_pref (24 B each: 12 KiB)
constexpr int kVpClBlock = 512;        // lanes of k_vp_cluster: one workgroup per image
constexpr int kVpLdsClusters = 2048;   // clusters whose state k_vp_cluster keeps in LDS (5 ints each: 40 KiB);
                                       // images with more valid lines keep it in global memory
constexpr int kVpStateInts = 5;        // per cluster: |P| (-1: merged away), partner, its intersection, its union, parent
constexpr int kVpMaxHypotheses = 1 << 20;

// one valid line: endpoints rounded to FP32 (JLinkage.cc:32-35) and widened again, midpoint, homogeneous coordinates
struct VpLine {
  double x1, y1, x2, y2;
  double cx, cy;
  double h0, h1, h2;
};
static_assert(sizeof(VpLine) == 72, "VpLine layout");

// an image that reaches the clustering: n valid lines at slot v0 of the scene's valid lines, its preference matrix at
// word p0 (word-major: word w of line k at p0 + w * n + k), its hypotheses at h0
struct VpImg {
  long long v0, p0, h0;
  int n, pad_;
};
static_assert(sizeof(VpImg) == 32, "VpImg layout");

// a k_vp_pref workgroup: lines [k0, k0 + kVpBlock) of image img, words [w0, w0 + kVpPrefWords)
struct VpBlock {
  int img, k0, w0, pad_;
};
static_assert(sizeof(VpBlock) == 16, "VpBlock layout");

struct VpHyp {
  double v0, v1, v2;
};

#define LT_VP_HD __host__ __device__ __forceinline__

// Line2d::length() (linebase.h:24): the norm of a 2-vector, x * x + y * y then the square root
LT_VP_HD double vp_length(double x1, double y1, double x2, double y2) {
  const double dx = x1 - x2, dy = y1 - y2;
  return sqrt(dx * dx + dy * dy);
}

LT_VP_HD VpLine vp_line(double x1, double y1, double x2, double y2) {
  VpLine r;
  r.x1 = (double)(float)x1; r.y1 = (double)(float)y1;
  r.x2 = (double)(float)x2; r.y2 = (double)(float)y2;
  r.cx = (r.x1 + r.x2) * 0.5;
  r.cy = (r.y1 + r.y2) * 0.5;
  r.h0 = r.y1 - r.y2;  // (x1, y1, 1) x (x2, y2, 1)
  r.h1 = r.x2 - r.x1;
  r.h2 = r.x1 * r.y2 - r.y1 * r.x2;
  return r;
}

// splitmix64 of seed * K + m; a = hi % n, b = (a + 1 + lo % (n - 1)) % n; n >= 2
LT_VP_HD void vp_sample(unsigned long long seed, unsigned long long m, unsigned n, unsigned *a, unsigned *b) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + m;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const unsigned hi = (unsigned)(z >> 32), lo = (unsigned)(z & 0xffffffffull);
  *a = hi % n;
  *b = (unsigned)(((unsigned long long)*a + 1ull + (unsigned long long)(lo % (n - 1))) % (unsigned long long)n);
}

LT_VP_HD VpHyp vp_hypothesis(const VpLine &p, const VpLine &q) {
  VpHyp v;
  v.v0 = p.h1 * q.h2 - p.h2 * q.h1;
  v.v1 = p.h2 * q.h0 - p.h0 * q.h2;
  v.v2 = p.h0 * q.h1 - p.h1 * q.h0;
  return v;
}

// Tardif's consistency of line l with the vanishing point v: the distance of an endpoint from the line through the
// midpoint and v.  A degenerate line gives NaN (or inf), which is no inlier
LT_VP_HD bool vp_inlier(double x1, double y1, double cx, double cy, const VpHyp &v, double th) {
  const double l0 = cy * v.v2 - v.v1;
  const double l1 = v.v0 - cx * v.v2;
  const double l2 = cx * v.v1 - cy * v.v0;
  const double err = fabs((l0 * x1 + l1 * y1) + l2) / sqrt(l0 * l0 + l1 * l1);
  return err <= th;
}

// the total order of the clustering: a pair with intersection c and union u beats another iff its ratio is greater
// (exactly, by cross-multiplication), then the smaller first index, then the smaller second index
LT_VP_HD bool vp_better(int c1, int u1, int i1, int j1, int c2, int u2, int i2, int j2) {
  const long long l = (long long)c1 * (long long)u2, r = (long long)c2 * (long long)u1;
  if (l != r) return l > r;
  if (i1 != i2) return i1 < i2;
  return j1 < j2;
}

// a launch carries its size per dimension (workgroups x lanes) in 32 bits: the callers keep every launch below 2^31
inline bool vp_launch_fits(long long workgroups, int lanes) { return workgroups <= (long long)INT_MAX / lanes; }

// flag[k] = !(length(line k) < min_length)
void launch_vp_prep(hipStream_t st, const double *lines4, long long n_lines, double min_length, unsigned char *flag);
// out[s] = vp_line(lines4[src[s]])
void launch_vp_lines(hipStream_t st, const double *lines4, const long long *src, long long n_valid, VpLine *out);
void launch_vp_hyp(hipStream_t st, const VpImg *imgs, int n_act, int n_hyp, unsigned long long seed, const VpLine *lines,
                   VpHyp *hyp);
void launch_vp_pref(hipStream_t st, const VpBlock *blk, int n_blk, const VpImg *imgs, int n_hyp, int n_words, double th,
                    const VpLine *lines, const VpHyp *hyp, unsigned long long *pref);
// roots[v0 + k] = the cluster (index of a valid line of the image) line k ends in; state: kVpStateInts ints per valid
// line of the scene, used by the images with more than kVpLdsClusters valid lines
void launch_vp_cluster(hipStream_t st, const VpImg *imgs, int n_act, int n_words, unsigned long long *pref, int *state,
                       int *roots);

}  // namespace lt
