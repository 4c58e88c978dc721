// lt_wunsch.h -- records and rules shared by the host side (lt_match_wunsch.cpp) and the device side
// (lt_kernels_wunsch.hip) of the SOLD2 line matcher (limap.line2d.SOLD2: WunschLineMatcher, model/line_matching.py).
// DESIGN §17, "SOLD2".  Everything here is one definition used on both sides: the pooling of an S x S block of point
// scores into a line score, and the Needleman-Wunsch value of a block.
#pragma once

#include "lt_match.h"

namespace lt {

constexpr int kWunschSlots = 8;       // point slots per line in the MFMA tile: num_samples real ones, zero rows behind
constexpr int kWunschTileLines = 4;   // lines per 32-row tile side (kMatchTile / kWunschSlots)
constexpr int kWunschMaxWaves = 4;    // waves per workgroup: each owns 4 lines of image 1
constexpr int kWunschMinSamples = 2, kWunschMaxSamples = 8;
constexpr int kWunschNwGroup = 16;    // lanes of k_wunsch_nw that share one line
constexpr float kWunschGap = 0.1f;    // needleman_wunsch: the gap penalty subtracted from every point score

// one (lines of image a) x (lines of image b) pair.  Point row (descriptor) s of line l of image a is row
// a0 + l * S + s of desc; its validity bit is bit s of vmask[la0 + l].  The kk best lines of b for every line of a go to
// slots [out0 + line * kk, +kk); the mutual form's match of a line to slot mout0 + line.
struct WunschTask {
  long long a0, b0, la0, lb0, out0, mout0;
  int na, nb, kk, pad_;  // na, nb: LINES
};
static_assert(sizeof(WunschTask) == 64, "WunschTask layout");

// The larger of two floats in the total order of match_key's score word (so -0.0f < +0.0f): the maxima of the pooling
// do not depend on the order in which lanes meet the values.
__host__ __device__ inline float wunsch_max(float x, float y) {
  int a, b;
#if defined(__HIP_DEVICE_COMPILE__)
  a = __float_as_int(x);
  b = __float_as_int(y);
#else
  std::memcpy(&a, &x, 4);
  std::memcpy(&b, &y, 4);
#endif
  const int ma = a ^ ((a >> 31) & 0x7fffffff), mb = b ^ ((b >> 31) & 0x7fffffff);
  return mb > ma ? y : x;
}

// "valid" is upstream's literal test: a maximum that equals -1.0f does not count, whatever produced it
__host__ __device__ inline float wunsch_term(float v) { return v != -1.0f ? v : 0.0f; }
__host__ __device__ inline int wunsch_counts(float v) { return v != -1.0f ? 1 : 0; }

// the mean of the counted maxima from the fixed tree's sum; a side without any counted maximum scores -1.0f
__host__ __device__ inline float wunsch_mean(float sum, int cnt) { return cnt ? sum / (float)cnt : -1.0f; }

// line score from the 8 slot maxima of either side (slots >= S hold -1.0f).  The sum is the fixed tree
// ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) over wunsch_term, FP32, no contraction.
__host__ __device__ inline float wunsch_pool8(const float v[8]) {
  int cnt = 0;
  float t[8];
  for (int k = 0; k < 8; ++k) {
    t[k] = wunsch_term(v[k]);
    cnt += wunsch_counts(v[k]);
  }
  const float lo = (t[0] + t[1]) + (t[2] + t[3]), hi = (t[4] + t[5]) + (t[6] + t[7]);
  return wunsch_mean(lo + hi, cnt);
}
__host__ __device__ inline float wunsch_line_score(float ls1, float ls2) { return (ls1 + ls2) * 0.5f; }

// Needleman-Wunsch value of one masked S x S block P (row s, column t at P[s * ld + t]): w = (double)(P - 0.1f),
// g[s+1][t+1] = max(max(g[s+1][t], g[s][t+1]), g[s][t] + w[s][t]) from zeros, in FP64; reversed: column S - 1 - t in
// place of t.  No cell is NaN (P is finite), so the maxima are plain comparisons.
template <int S>
__host__ __device__ inline double wunsch_nw(const float *P, int ld, bool reversed) {
  double row[S + 1];
  for (int t = 0; t <= S; ++t) row[t] = 0.0;
  for (int s = 0; s < S; ++s) {
    double diag = 0.0;  // g[s][t]
    row[0] = 0.0;
    for (int t = 0; t < S; ++t) {
      const float p = P[s * ld + (reversed ? S - 1 - t : t)];
      const double w = (double)(p - kWunschGap);
      const double up = row[t + 1], left = row[t];
      const double m = left > up ? left : up;
      const double d = diag + w;
      diag = up;
      row[t + 1] = d > m ? d : m;
    }
  }
  return row[S];
}

// kernel 1: line scores by the FP32-input MFMA, pooled in the accumulator layout, top-kk lines per line
void launch_wunsch_topk(hipStream_t st, int dim, int S, int kcap, int waves, const WunschTask *tasks,
                        const MatchUnit *units, int n_units, const float *desc, const unsigned char *vmask,
                        unsigned short *out_col, float *out_score);
// kernel 2: per (task, line) the NW values of its kk candidates in both orientations; the first maximum's candidate
// and its line score go to mcol / mscore[mout0 + line].  prefix[t] = lines of the tasks before t (n_tasks + 1 entries).
void launch_wunsch_nw(hipStream_t st, int dim, int S, const WunschTask *tasks, const long long *prefix, int n_tasks,
                      long long n_lines, const float *desc, const unsigned char *vmask, const unsigned short *col,
                      const float *score, unsigned short *mcol, float *mscore);
// cross check: tasks [0, n_pairs) forward, [n_pairs, 2 n_pairs) swapped; mcol of a forward line becomes 0xffff where
// the match of its match is another line
void launch_wunsch_mutual(hipStream_t st, const WunschTask *tasks, int n_pairs, unsigned short *mcol);

}  // namespace lt
