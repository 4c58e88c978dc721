// lt_dense.h -- records and rules shared by the host side (lt_match_dense.cpp) and the device side
// (lt_kernels_dense.hip) of the dense-warp line matcher (limap.line2d.dense: BaseDenseLineMatcher, dense/matcher.py).
// DESIGN §17, "Dense".  Everything here is one definition used on both sides: the sample of a line, the bilinear tap of
// the warp, one direction's (weighted distance, overlap) of an entry and the combination of the two directions.  FP32,
// no contraction (-ffp-contract=off on both compilers), every fused operation an explicit fmaf.
#pragma once

#include "lt_match.h"

#include <cfloat>
#include <cmath>

namespace lt {

constexpr int kDenseTile = 16;            // k_dense_pairs: 16 lines of image 1 x 16 lines of image 2, one entry per lane
constexpr int kDenseMinSamples = 2, kDenseMaxSamples = 64;  // a line's good flags are one 64-bit word
constexpr int kDenseMaxWarpDim = 16384;   // texels per side of a warp (a tap index stays below 2^28)
constexpr float kDenseFar = 10000.0f;     // upstream's "no overlap" distance
// the tables of a call, one float array: r_k (S), overlap by count (S + 1), 1 / count by count (S + 1)
constexpr int kDenseTabR = 0, kDenseTabOvl = 64, kDenseTabInv = 64 + 65, kDenseTabLen = 64 + 65 + 65;

// what a target line contributes, prepared once per image on the host: unit direction, the projections of its two ends
// on it, the homogeneous line over the norm of its first two components
struct DenseLine {
  float dx, dy, sp, ep, lx, ly, lz, pad_;
};
static_assert(sizeof(DenseLine) == 32, "DenseLine layout");

// one direction of one pair: the n lines [src0, src0 + n) go through warp (hw, ww, 2) / cert (hw, ww); sample k of line l
// lands in slot smp0 + k * n + l of the warped arrays
struct DenseDir {
  const float *warp, *cert;
  long long src0, smp0;
  int n, hw, ww, pad_;
  float ax, ay;  // (float)(2.0 / w), (float)(2.0 / h) of the source image
  float tw, th;  // (float)w, (float)h of the target image
};
static_assert(sizeof(DenseDir) == 64, "DenseDir layout");

// one pair: lines [a0, a0 + n1) of image 1, [b0, b0 + n2) of image 2; its entries at d0 + i * n2 + j, its rows'
// counters at r0 + i
struct DenseTask {
  long long a0, b0, s12, s21, d0, r0;
  int n1, n2;
};
static_assert(sizeof(DenseTask) == 56, "DenseTask layout");

struct DenseUnit {  // a workgroup of k_dense_pairs: the tile at (i0, j0) of a task
  int task, i0, j0;
};

__host__ __device__ inline bool dense_finite(float v) { return fabsf(v) <= FLT_MAX; }

// sample k of the line (sx, sy, ex, ey): r start + (1 - r) end -- one subtraction, two products and one sum per
// coordinate (dense/matcher.py:58-66: r = 0 is the END of the line)
__host__ __device__ inline void dense_sample(const float *ln, float r, float &x, float &y) {
  const float q = 1.0f - r;
  const float ax = r * ln[0], bx = q * ln[2], ay = r * ln[1], by = q * ln[3];
  x = ax + bx;
  y = ay + by;
}

// the four taps of grid_sample(mode="bilinear", align_corners=False, padding_mode="zeros") at the normalised point
// (xn, yn) of an (H, W) map, in the order nw, ne, sw, se.  A tap outside the map (or of a non-finite point) is absent.
struct DenseTaps {
  int idx[4];
  float w[4];
  bool in[4];
};
__host__ __device__ inline void dense_taps(float xn, float yn, int H, int W, DenseTaps &t) {
  const float ix = ((xn + 1.0f) * (float)W - 1.0f) * 0.5f;
  const float iy = ((yn + 1.0f) * (float)H - 1.0f) * 0.5f;
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float we = ix - x0, ww = x1 - ix, ws = iy - y0, wn = y1 - iy;
  t.w[0] = ww * wn;
  t.w[1] = we * wn;
  t.w[2] = ww * ws;
  t.w[3] = we * ws;
  const float xm = (float)(W - 1), ym = (float)(H - 1);
  const bool x0in = x0 >= 0.0f && x0 <= xm, x1in = x1 >= 0.0f && x1 <= xm;  // (false for NaN)
  const bool y0in = y0 >= 0.0f && y0 <= ym, y1in = y1 >= 0.0f && y1 <= ym;
  const int xi0 = x0in ? (int)x0 : 0, xi1 = x1in ? (int)x1 : 0, yi0 = y0in ? (int)y0 : 0, yi1 = y1in ? (int)y1 : 0;
  t.in[0] = x0in && y0in;
  t.in[1] = x1in && y0in;
  t.in[2] = x0in && y1in;
  t.in[3] = x1in && y1in;
  t.idx[0] = yi0 * W + xi0;
  t.idx[1] = yi0 * W + xi1;
  t.idx[2] = yi1 * W + xi0;
  t.idx[3] = yi1 * W + xi1;
}
// the interpolated value of one channel: the fmaf chain over the present taps in their order, from +0.0f
__host__ __device__ inline float dense_gather(const float *p, int stride, const DenseTaps &t) {
  float acc = 0.0f;
  for (int q = 0; q < 4; ++q)
    if (t.in[q]) acc = fmaf(p[(long long)t.idx[q] * stride], t.w[q], acc);
  return acc;
}

// the point (xs, ys) of the source image through one direction: target coordinates and whether the sample's certainty
// passes.  A non-finite coordinate or certainty is never good.
__host__ __device__ inline bool dense_warp_point(const float *warp, const float *cert, int hw, int ww, float ax, float ay,
                                                 float tw, float th, float thresh, float xs, float ys, float &x,
                                                 float &y) {
  const float xn = ax * xs - 1.0f, yn = ay * ys - 1.0f;
  DenseTaps t;
  dense_taps(xn, yn, hw, ww, t);
  const float wx = dense_gather(warp, 2, t), wy = dense_gather(warp + 1, 2, t), c = dense_gather(cert, 1, t);
  x = ((wx + 1.0f) * tw) * 0.5f;
  y = ((wy + 1.0f) * th) * 0.5f;
  return c > thresh && dense_finite(c) && dense_finite(x) && dense_finite(y);
}

__host__ __device__ inline int dense_popc(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// one direction of one entry: the S warped samples px[k * stride], py[k * stride] of a line with certainty word m against
// the target line L.  ovl / inv: the tables by count.  d: the weighted distance (kDenseFar below seg_th), o: the overlap.
__host__ __device__ inline void dense_direction(const float *px, const float *py, int stride, unsigned long long m,
                                                const DenseLine &L, int S, const float *ovl, const float *inv,
                                                float seg_th, float &d, float &o) {
  unsigned long long g = 0ull;
  for (int k = 0; k < S; ++k) {
    const float x = px[k * stride], y = py[k * stride];
    const float proj = fmaf(y, L.dy, x * L.dx);
    if (proj > L.sp && proj < L.ep) g |= 1ull << k;
  }
  g &= m;
  const int cnt = dense_popc(g);
  const float w = inv[cnt];
  float acc = 0.0f;
  for (int k = 0; k < S; ++k)
    if ((g >> k) & 1ull) {
      const float x = px[k * stride], y = py[k * stride];
      const float dist = fabsf(fmaf(y, L.ly, x * L.lx) + L.lz);
      acc = fmaf(dist, w, acc);
    }
  o = ovl[cnt];
  d = o < seg_th ? kDenseFar : acc;
}

// dense/matcher.py:172-182
__host__ __device__ inline float dense_combine(float d12, float o12, float d21, float o21, float seg_th, float pix_th) {
  float d = o12 > o21 ? d12 : d21;
  const float omin = o21 < o12 ? o21 : o12;
  if (omin < seg_th) d = kDenseFar;
  const float dmax = d21 > d12 ? d21 : d12;
  if (dmax > pix_th) d = kDenseFar;
  return d;
}

// kernel 1: one lane per (direction, sample): the warped coordinate and the certainty flag of every sample
void launch_dense_warp(hipStream_t st, const DenseDir *dirs, int n_dirs, int max_n, int S, float thresh,
                       const float *lines, const float *tab, float *wx, float *wy, unsigned char *wok);
// kernel 2: one entry of dists per lane, a 16 x 16 tile per workgroup; aux (may be null): d12, o12, d21, o21 of every
// entry behind each other, `total` floats each
void launch_dense_pairs(hipStream_t st, const DenseTask *tasks, const DenseUnit *units, int n_units, int S, float seg_th,
                        float pix_th, const DenseLine *terms, const float *tab, const float *wx, const float *wy,
                        const unsigned char *wok, float *dists, float *aux, long long total);
// kernel 3: a wave per line of image 1.  fill == 0: cnt[r0 + i] = its rows; fill != 0: the rows at off[r0 + i]
void launch_dense_select(hipStream_t st, const DenseTask *tasks, int n_tasks, int max_n1, int fill, int one_to_many,
                         float pix_th, const float *dists, unsigned *cnt, const long long *off, int *out_line,
                         unsigned short *out_col, float *out_score);

}  // namespace lt
