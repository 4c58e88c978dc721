// lt_kernels_match.hip -- line-descriptor matching on the device: per (image, neighbour) pair the score
// matrix desc1 . desc2^T by the FP32-input MFMA, and the top-k columns of every line selected on chip.  The score matrix
// never reaches memory.
//
// score(i, j) is the fmaf chain over the descriptor dimension in ascending k from +0.0f.  v_mfma_f32_32x32x2_f32 computes
// exactly that chain when every k-step accumulates into the same accumulator, so the K-loop below has ONE accumulator
// tile per wave; independence between waves comes from different output tiles, never from splitting K.
//
// Orientation: the MFMA's A operand is the column tile (32 descriptor rows of image 2, from LDS), its B operand the
// wave's 32 rows of image 1 (registers, loaded once per workgroup).  D[i][j] then has j = the image-1 row on the lane
// (lane & 31) and the 16 image-2 columns i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in the lane's registers: a lane
// scans the scores of its own row without any transpose.
//
// Selection: every lane keeps the best `kcap` keys (match_key: score bits, ~column) of the columns it has seen, sorted,
// in LDS.  The key is a total order, so the best kcap of a row are the best kcap of the union of its two lanes' lists
// whatever the tiling; the two lists are merged at the end.  No atomics.

#include "lt_match.h"

namespace lt {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

__device__ inline void list_insert(u64 *list, int kcap, int &cnt, u64 &thr, u64 key) {
  int p;
  if (cnt < kcap) p = cnt++;
  else p = kcap - 1;
  while (p > 0) {
    const u64 prev = list[(p - 1) * 64];
    if (prev > key) break;
    list[p * 64] = prev;
    --p;
  }
  list[p * 64] = key;
  thr = (cnt == kcap) ? list[(kcap - 1) * 64] : 0ull;
}

// HALF: k-steps held in registers per lane (dim <= 2 * HALF).  KIND 0: L2D2 (a descriptor row is a line); KIND 1:
// endpoints (rows 2 i, 2 i + 1 are the endpoints of line i).
template <int HALF, int KIND>
__global__ void __launch_bounds__(64 * kMatchMaxWaves)
k_match_topk(const MatchTask *__restrict__ tasks, const MatchUnit *__restrict__ units, const float *__restrict__ desc,
             int dim, int kcap, unsigned short *__restrict__ out_col, float *__restrict__ out_score) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int waves = (int)blockDim.x >> 6;
  const int stride = dim + kMatchPad, half = dim >> 1;
  float *sB = reinterpret_cast<float *>(smem);                                       // [32][stride], k permuted
  u64 *lists = reinterpret_cast<u64 *>(smem + sizeof(float) * kMatchTile * stride);  // [wave][slot][lane]

  const MatchUnit unit = units[blockIdx.x];
  const MatchTask T = tasks[unit.task];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int row = unit.row0 + wave * kMatchTile + r;  // descriptor row of image a
  const bool row_ok = row < T.na;
  u64 *my = lists + (size_t)wave * kcap * 64 + lane;

  // this lane's k-steps of its row: k = 2 s + h
  float ra[HALF];
  {
    const float4 *src = reinterpret_cast<const float4 *>(desc + (T.a0 + (row_ok ? row : 0)) * (long long)dim);
#pragma unroll
    for (int t = 0; t < HALF / 2; ++t) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * t < dim && row_ok) v = src[t];
      ra[2 * t] = h ? v.y : v.x;
      ra[2 * t + 1] = h ? v.w : v.z;
    }
  }

  int cnt = 0;
  u64 thr = 0ull;
  const int q4 = dim >> 2;  // float4 per descriptor row
  for (int col0 = 0; col0 < T.nb; col0 += kMatchTile) {
    __syncthreads();  // the previous tile has been read
    // stage 32 rows of image b, position of k: (k & 1) * half + (k >> 1); rows past the image are zeros
    for (int e = tid; e < kMatchTile * q4; e += (int)blockDim.x) {
      const int c = e / q4, u = e - c * q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col0 + c < T.nb) v = reinterpret_cast<const float4 *>(desc + (T.b0 + col0 + c) * (long long)dim)[u];
      float *dst = sB + c * stride;
      *reinterpret_cast<float2 *>(dst + 2 * u) = make_float2(v.x, v.z);
      *reinterpret_cast<float2 *>(dst + half + 2 * u) = make_float2(v.y, v.w);
    }
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const float4 *bp = reinterpret_cast<const float4 *>(sB + r * stride + h * half);
#pragma unroll
    for (int t = 0; t < HALF / 4; ++t) {
      if (8 * t < dim) {  // (uniform)
        const float4 b = bp[t];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, ra[4 * t], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, ra[4 * t + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, ra[4 * t + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, ra[4 * t + 3], acc, 0, 0, 0);
      }
    }

    if (KIND == 0) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int col = col0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (row_ok && col < T.nb) {
          const u64 key = match_key(acc[q], (unsigned)col);
          if (key > thr) list_insert(my, kcap, cnt, thr, key);
        }
      }
    } else {
      // the other endpoint of this lane's line is on the neighbouring lane; the even lane of a pair selects
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        const float p0 = __shfl_xor(acc[q], 1), p1 = __shfl_xor(acc[q + 1], 1);
        const int col = col0 + (q & 3) + 8 * (q >> 2) + 4 * h;  // even: endpoint 0 of line col / 2
        if (!(r & 1) && row_ok && col < T.nb) {
          const float s = match_endpoint_score(acc[q], p1, acc[q + 1], p0);
          const u64 key = match_key(s, (unsigned)(col >> 1));
          if (key > thr) list_insert(my, kcap, cnt, thr, key);
        }
      }
    }
  }

  // merge the lists of lanes r and r + 32: the kk best of the row, best first
  const int cnt_hi = __shfl(cnt, r + 32);
  const bool owner = h == 0 && row_ok && (KIND == 0 || !(r & 1));
  if (owner) {
    const u64 *la = my, *lb = my + 32;
    const long long line = KIND == 0 ? row : (row >> 1);
    const long long o = T.out0 + line * T.kk;
    int ia = 0, ib = 0;
    for (int t = 0; t < T.kk; ++t) {
      const u64 ka = ia < cnt ? la[ia * 64] : 0ull, kb = ib < cnt_hi ? lb[ib * 64] : 0ull;
      u64 best;
      if (ka > kb) { best = ka; ++ia; }
      else { best = kb; ++ib; }
      out_col[o + t] = (unsigned short)match_key_col(best);
      out_score[o + t] = match_key_score(best);
    }
  }
}

__global__ void k_match_check(const float *__restrict__ desc, long long n, int *flag) {
  bool bad = false;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    const float v = desc[k];
    if (!(fabsf(v) <= kMatchMaxAbs)) bad = true;
  }
  if (bad) *flag = 1;  // (every writer stores the same value)
}

// one workgroup per pair: line i keeps its best column j only if i is the best line of j
__global__ void k_match_mutual(const MatchTask *__restrict__ tasks, int n_pairs, int rows_per_line,
                               unsigned short *col) {
  const MatchTask F = tasks[blockIdx.x], B = tasks[n_pairs + blockIdx.x];
  const int lines = F.na / rows_per_line;
  if (F.nb == 0) return;
  for (int i = (int)threadIdx.x; i < lines; i += (int)blockDim.x) {
    const unsigned j = col[F.out0 + i];  // (slot i is read and written by this thread alone)
    col[F.out0 + i] = (col[B.out0 + j] == (unsigned)i) ? (unsigned short)j : (unsigned short)0xffff;
  }
}

}  // namespace

int match_waves(int dim, int kcap) {
  int w = kMatchMaxWaves;
  while (w > 1 && match_lds_bytes(dim, kcap, w) > 96 * 1024) w >>= 1;
  return w;
}

size_t match_lds_bytes(int dim, int kcap, int waves) {
  return sizeof(float) * kMatchTile * (size_t)(dim + kMatchPad) + sizeof(u64) * 64 * (size_t)kcap * (size_t)waves;
}

void launch_match_check(hipStream_t st, const float *desc, long long n, int *flag) {
  if (n <= 0) return;
  const int blocks = (int)((n + 256 * 16 - 1) / (256 * 16));
  hipLaunchKernelGGL(k_match_check, dim3(blocks > 4096 ? 4096 : blocks), dim3(256), 0, st, desc, n, flag);
}

void launch_match_topk(hipStream_t st, int kind, int dim, int kcap, int waves, const MatchTask *tasks,
                       const MatchUnit *units, int n_units, const float *desc, unsigned short *out_col,
                       float *out_score) {
  if (n_units <= 0) return;
  const size_t lds = match_lds_bytes(dim, kcap, waves);
  const dim3 grid((unsigned)n_units), block(64u * (unsigned)waves);
#define LT_MATCH_LAUNCH(H, K)                                                                                    \
  do {                                                                                                           \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_match_topk<H, K>),                               \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                             \
    hipLaunchKernelGGL((k_match_topk<H, K>), grid, block, lds, st, tasks, units, desc, dim, kcap, out_col,       \
                       out_score);                                                                               \
  } while (0)
  if (dim <= 128) {
    if (kind == 0) LT_MATCH_LAUNCH(64, 0);
    else LT_MATCH_LAUNCH(64, 1);
  } else {
    if (kind == 0) LT_MATCH_LAUNCH(128, 0);
    else LT_MATCH_LAUNCH(128, 1);
  }
#undef LT_MATCH_LAUNCH
}

void launch_match_mutual(hipStream_t st, const MatchTask *tasks, int n_pairs, int rows_per_line, unsigned short *col) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL(k_match_mutual, dim3((unsigned)n_pairs), dim3(256), 0, st, tasks, n_pairs, rows_per_line, col);
}

}  // namespace lt
