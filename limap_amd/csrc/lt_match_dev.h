// lt_match_dev.h -- the device core shared by k_match_topk (lt_kernels_match.hip) and k_wunsch_topk
// (lt_kernels_wunsch.hip): the MFMA score tile and the on-chip top-k of DESIGN §17, and the mutual cross check.  Only
// those two files include it.
//
// score(i, j) is the fmaf chain over the descriptor dimension in ascending k from +0.0f.  v_mfma_f32_32x32x2_f32 computes
// exactly that chain when every k-step accumulates into the same accumulator, so mfma_tile has ONE accumulator tile per
// wave; independence between waves comes from different output tiles, never from splitting K.
//
// Orientation: the MFMA's A operand is the column tile (32 descriptor rows of image 2, from LDS), its B operand the
// wave's 32 rows of image 1 (registers, loaded once per workgroup).  D[i][j] then has j = the image-1 row on the lane
// (lane & 31) and the 16 image-2 columns i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in the lane's registers: a lane
// scans the scores of its own row without any transpose.
//
// LDS: sB [32][dim + kMatchPad] floats, the column tile with k at position (k & 1) * dim/2 + (k >> 1), so that the
// k-steps of a lane half are contiguous; behind it the key lists [wave][slot][list], STRIDE lists per wave.
//
// Selection: a list keeps the best `kcap` keys (match_key: score bits, ~column) of the columns its lane has seen,
// sorted.  The key is a total order, so the best kcap of a row are the best kcap of the union of the two lists that saw
// its columns whatever the tiling; merge_lists joins them at the end.  No atomics.
#pragma once

#include "lt_match.h"

namespace lt {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

// dynamic LDS of a top-k kernel: the column tile and `lists` key lists of kcap slots per wave
inline size_t topk_lds_bytes(int dim, int kcap, int waves, int lists) {
  return sizeof(float) * kMatchTile * (size_t)(dim + kMatchPad) + sizeof(u64) * (size_t)lists * (size_t)kcap * (size_t)waves;
}

// `key` into a sorted list whose slots lie STRIDE apart; thr becomes the kcap-th key once the list is full
template <int STRIDE>
__device__ __forceinline__ void topk_insert(u64 *list, int kcap, int &cnt, u64 &thr, u64 key) {
  int p;
  if (cnt < kcap) p = cnt++;
  else p = kcap - 1;
  while (p > 0) {
    const u64 prev = list[(p - 1) * STRIDE];
    if (prev > key) break;
    list[p * STRIDE] = prev;
    --p;
  }
  list[p * STRIDE] = key;
  thr = (cnt == kcap) ? list[(kcap - 1) * STRIDE] : 0ull;
}

// lane half h's k-steps of its image-1 row: k = 2 s + h (HALF: k-steps held per lane, dim <= 2 * HALF); zeros when
// the row does not exist
template <int HALF>
__device__ __forceinline__ void load_row(const float *row, int dim, bool row_ok, int h, float (&ra)[HALF]) {
  const float4 *src = reinterpret_cast<const float4 *>(row);
#pragma unroll
  for (int t = 0; t < HALF / 2; ++t) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * t < dim && row_ok) v = src[t];
    ra[2 * t] = h ? v.y : v.x;
    ra[2 * t + 1] = h ? v.w : v.z;
  }
}

// the workgroup stages the 32-row column tile between two barriers; row_of(c, src) sets src to the descriptor row
// behind tile row c and returns false where the row is zeros (the test stays apart from the pointer: a null test on a
// computed address costs the 256-wide forms SGPRs they do not have).  threads: blockDim.x, read by the kernel ahead
// of its tile loop -- read here, its scalar load and the wait for it land in every tile.
template <class RowOf>
__device__ __forceinline__ void stage_tile(float *sB, int dim, int threads, RowOf row_of) {
  const int stride = dim + kMatchPad, half = dim >> 1, q4 = dim >> 2;  // q4: float4 per descriptor row
  __syncthreads();  // the previous tile has been read
  for (int e = (int)threadIdx.x; e < kMatchTile * q4; e += threads) {
    const int c = e / q4, u = e - c * q4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *src;
    if (row_of(c, src)) v = reinterpret_cast<const float4 *>(src)[u];
    float *dst = sB + c * stride;
    *reinterpret_cast<float2 *>(dst + 2 * u) = make_float2(v.x, v.z);
    *reinterpret_cast<float2 *>(dst + half + 2 * u) = make_float2(v.y, v.w);
  }
  __syncthreads();
}

// the score tile: bp = the lane's tile row and half in sB, ra = its image-1 k-steps; one accumulator, ascending k
template <int HALF>
__device__ __forceinline__ f32x16 mfma_tile(const float4 *bp, const float (&ra)[HALF], int dim) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
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
  return acc;
}

// Called by every lane of the wave.  An owner (a lane with h == 0) merges its list la with lb, the list of lane + 32,
// and writes the kk best, best first.  lb was written by another lane of this wave, and from one thread's view its
// slots never alias the thread's own: the fence and the barrier order those stores before the loads below.
template <int STRIDE>
__device__ __forceinline__ void merge_lists(bool owner, const u64 *la, const u64 *lb, int cnt, int kk,
                                            unsigned short *out_col, float *out_score) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int cnt_hi = __shfl(cnt, ((int)threadIdx.x & 31) + 32);
  if (!owner) return;
  int ia = 0, ib = 0;
  for (int t = 0; t < kk; ++t) {
    const u64 ka = ia < cnt ? la[ia * STRIDE] : 0ull, kb = ib < cnt_hi ? lb[ib * STRIDE] : 0ull;
    u64 best;
    if (ka > kb) { best = ka; ++ia; }
    else { best = kb; ++ib; }
    out_col[t] = (unsigned short)match_key_col(best);
    out_score[t] = match_key_score(best);
  }
}

// The cross check, one workgroup per pair: tasks [0, n_pairs) are (image, neighbour), [n_pairs, 2 n_pairs) the same
// pairs swapped; OUT0 names the first slot of a task's line matches in col.  Line i keeps its match j only if the match
// of j is i.
template <class Task, long long Task::*OUT0>
__global__ void k_mutual(const Task *__restrict__ tasks, int n_pairs, int rows_per_line, unsigned short *col) {
  const Task F = tasks[blockIdx.x], B = tasks[n_pairs + blockIdx.x];
  if (F.kk == 0) return;
  const int lines = F.na / rows_per_line;
  for (int i = (int)threadIdx.x; i < lines; i += (int)blockDim.x) {
    const unsigned j = col[F.*OUT0 + i];  // (slot i is read and written by this thread alone)
    col[F.*OUT0 + i] = (col[B.*OUT0 + j] == (unsigned)i) ? (unsigned short)j : (unsigned short)0xffff;
  }
}

template <class Task, long long Task::*OUT0>
void launch_mutual(hipStream_t st, const Task *tasks, int n_pairs, int rows_per_line, unsigned short *col) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL((k_mutual<Task, OUT0>), dim3((unsigned)n_pairs), dim3(256), 0, st, tasks, n_pairs, rows_per_line, col);
}

}  // namespace

}  // namespace lt
