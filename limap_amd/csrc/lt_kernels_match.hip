// lt_kernels_match.hip -- line-descriptor matching on the device: per (image, neighbour) pair the score
// matrix desc1 . desc2^T by the FP32-input MFMA, and the top-k columns of every line selected on chip.  The score matrix
// never reaches memory.  The score tile, the key lists and the cross check are the shared core of lt_match_dev.h; here
// are the two kinds' mapping of scores to lines and the input check.

#include "lt_match_dev.h"

namespace lt {

namespace {

// HALF: k-steps held in registers per lane (dim <= 2 * HALF).  KIND 0: L2D2 (a descriptor row is a line); KIND 1:
// endpoints (rows 2 i, 2 i + 1 are the endpoints of line i).
template <int HALF, int KIND>
__global__ void __launch_bounds__(64 * kMatchMaxWaves)
k_match_topk(const MatchTask *__restrict__ tasks, const MatchUnit *__restrict__ units, const float *__restrict__ desc,
             int dim, int kcap, unsigned short *__restrict__ out_col, float *__restrict__ out_score) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int threads = (int)blockDim.x, stride = dim + kMatchPad, half = dim >> 1;
  float *sB = reinterpret_cast<float *>(smem);                                       // [32][stride], k permuted
  u64 *lists = reinterpret_cast<u64 *>(smem + sizeof(float) * kMatchTile * stride);  // [wave][slot][lane]

  const MatchUnit unit = units[blockIdx.x];
  const MatchTask T = tasks[unit.task];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int row = unit.row0 + wave * kMatchTile + r;  // descriptor row of image a
  const bool row_ok = row < T.na;
  u64 *my = lists + (size_t)wave * kcap * 64 + lane;

  float ra[HALF];  // this lane's k-steps of its row
  load_row<HALF>(desc + (T.a0 + (row_ok ? row : 0)) * (long long)dim, dim, row_ok, h, ra);

  int cnt = 0;
  u64 thr = 0ull;
  for (int col0 = 0; col0 < T.nb; col0 += kMatchTile) {
    // 32 rows of image b; rows past the image are zeros
    stage_tile(sB, dim, threads, [&](int c, const float *&src) {
      src = desc + (T.b0 + col0 + c) * (long long)dim;
      return col0 + c < T.nb;
    });
    const f32x16 acc = mfma_tile<HALF>(reinterpret_cast<const float4 *>(sB + r * stride + h * half), ra, dim);

    if (KIND == 0) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int col = col0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (row_ok && col < T.nb) {
          const u64 key = match_key(acc[q], (unsigned)col);
          if (key > thr) topk_insert<64>(my, kcap, cnt, thr, key);
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
          if (key > thr) topk_insert<64>(my, kcap, cnt, thr, key);
        }
      }
    }
  }

  // the lists of lanes r and r + 32 hold the row's columns: its kk best, best first
  const bool owner = h == 0 && row_ok && (KIND == 0 || !(r & 1));
  const long long o = T.out0 + (long long)(KIND == 0 ? row : (row >> 1)) * T.kk;
  merge_lists<64>(owner, my, my + 32, cnt, T.kk, out_col + o, out_score + o);
}

__global__ void k_match_check(const float *__restrict__ desc, long long n, int *flag) {
  bool bad = false;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    const float v = desc[k];
    if (!(fabsf(v) <= kMatchMaxAbs)) bad = true;
  }
  if (bad) *flag = 1;  // (every writer stores the same value)
}

}  // namespace

int match_waves(int dim, int kcap) {
  int w = kMatchMaxWaves;
  while (w > 1 && match_lds_bytes(dim, kcap, w) > 96 * 1024) w >>= 1;
  return w;
}

size_t match_lds_bytes(int dim, int kcap, int waves) { return topk_lds_bytes(dim, kcap, waves, 64); }

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
  launch_mutual<MatchTask, &MatchTask::out0>(st, tasks, n_pairs, rows_per_line, col);
}

}  // namespace lt
