// lt_match.h -- records and rules shared by the host side (lt_match.cpp) and the device side (lt_kernels_match.hip)
// of line-descriptor matching (limap.line2d: L2D2Matcher, NNEndpointsMatcher top-k; line2d/L2D2/matcher.py,
// line2d/endpoints/matcher.py:71-111).  DESIGN §17.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

namespace lt {

constexpr int kMatchTile = 32;        // descriptor rows per MFMA tile side (v_mfma_f32_32x32x2_f32)
constexpr int kMatchMaxWaves = 4;     // waves per workgroup: each owns kMatchTile rows of image 1, all share a column tile
constexpr int kMatchMaxDim = 256;     // descriptor width: a multiple of 8 in [8, 256]
constexpr int kMatchMaxTopk = 64;     // LT_MATCH_MAX_TOPK
constexpr int kMatchPad = 4;          // floats between the rows of the column tile in LDS
constexpr int kMatchMaxLines = 65535; // lines per image (the triangulator's limit); 0xffff marks "no match"
constexpr float kMatchMaxAbs = 0x1p57f;  // |descriptor value| bound: no score can overflow (256 * 2 * 2^114 < 2^128)

// one (rows of image a) x (rows of image b) contraction: descriptor rows [a0, a0 + na) against [b0, b0 + nb); the
// kk best of every line of a go to slots [out0 + line * kk, +kk)
struct MatchTask {
  long long a0, b0, out0;
  int na, nb, kk, pad_;
};
static_assert(sizeof(MatchTask) == 40, "MatchTask layout");

// a workgroup's share: descriptor rows [row0, row0 + 32 * waves) of task `task`
struct MatchUnit {
  int task, row0;
};

// The total order of the selection: larger key = better.  High word: the score's bits made monotone (negative floats
// reversed); low word: ~column, so that equal scores rank by ascending column.  Keys are never 0.
__host__ __device__ inline unsigned long long match_key(float score, unsigned col) {
  unsigned u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(score);
#else
  std::memcpy(&u, &score, 4);
#endif
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - col);
}
__host__ __device__ inline float match_key_score(unsigned long long key) {
  unsigned u = (unsigned)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(u);
#else
  std::memcpy(&f, &u, 4);
#endif
  return f;
}
__host__ __device__ inline unsigned match_key_col(unsigned long long key) { return 0xffffffffu - (unsigned)key; }

// line score of the endpoints matcher from the four point scores (endpoints/matcher.py:95-98): two FP32 additions, the
// larger of the two (the first when they are equal: fmaxf leaves the sign of a zero open), times one half
__host__ __device__ inline float match_endpoint_score(float s00, float s11, float s01, float s10) {
  const float x = s00 + s11, y = s01 + s10;
  const float m = (y > x) ? y : x;
  return 0.5f * m;
}

// waves per workgroup and dynamic LDS bytes of k_match_topk for a descriptor width and a list length
int match_waves(int dim, int kcap);
size_t match_lds_bytes(int dim, int kcap, int waves);
// flag[0] = 1 when a value is not finite or above kMatchMaxAbs in magnitude
void launch_match_check(hipStream_t st, const float *desc, long long n, int *flag);
// kind 0: a line per descriptor row; kind 1: two rows (endpoints) per line.  out_col / out_score: per output slot
void launch_match_topk(hipStream_t st, int kind, int dim, int kcap, int waves, const MatchTask *tasks,
                       const MatchUnit *units, int n_units, const float *desc, unsigned short *out_col,
                       float *out_score);
// mutual nearest neighbours: tasks [0, n_pairs) are (image, neighbour), [n_pairs, 2 n_pairs) the same pairs swapped,
// all with kk = 1; out_col[out0 + i] of the first half becomes 0xffff where line i is not its best column's best line
void launch_match_mutual(hipStream_t st, const MatchTask *tasks, int n_pairs, int rows_per_line, unsigned short *col);

}  // namespace lt
