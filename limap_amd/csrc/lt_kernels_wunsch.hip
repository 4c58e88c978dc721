// lt_kernels_wunsch.hip -- the SOLD2 line matcher on the device ("SOLD2"): per (image, neighbour) pair the
// point-score matrix P by the FP32-input MFMA, every num_samples x num_samples block pooled into a line score in the
// accumulator's own layout, the top-k lines of every line selected on chip (k_wunsch_topk); and, for the mutual form,
// the Needleman-Wunsch values of every line's candidates in both orientations (k_wunsch_nw) with the cross check
// (k_mutual).  Neither P nor the line scores reach memory.
//
// Tile layout.  Every line has 8 point slots: its S samples, then zero rows.  A 32 x 32 MFMA tile therefore holds
// 4 x 4 whole line blocks.  The score tile and the key lists are the core of lt_match_dev.h, shared with k_match_topk:
// the A operand is the tile of image 2 (LDS), the B operand the wave's 32 point slots of image 1 (registers); lane l
// owns slot r = l & 31 of image 1 -- line r >> 3, sample s = r & 7 -- and its register q the image-2 slot
// (q & 3) + 8 (q >> 2) + 4 (l >> 5): line q >> 2, sample t = (q & 3) + 4 (l >> 5).  So
//   max over t  = four registers and the partner lane l ^ 32 (a slot pair past S is absent: -inf never wins),
//   max over s  = three cross-lane steps inside 8 consecutive lanes,
//   the sums    = the same two patterns: the fixed tree ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) of wunsch_pool8.
// Every cross-lane step is a butterfly of a commutative operation, so all lanes of a line end with the same bits.

#include "lt_match_dev.h"
#include "lt_wunsch.h"

namespace lt {

namespace {

constexpr int kListStride = 2 * kWunschTileLines;  // lists per wave: (line of the wave, half)

// sum / count / maximum over the 8 lanes of a line (lanes that differ in bits 0..2)
__device__ inline float sum8(float v) {
  v = v + __shfl_xor(v, 1);
  v = v + __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}
__device__ inline int cnt8(int v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}
__device__ inline float max8(float v) {
  v = wunsch_max(v, __shfl_xor(v, 1));
  v = wunsch_max(v, __shfl_xor(v, 2));
  return wunsch_max(v, __shfl_xor(v, 4));
}

// the value of a slot pair that does not exist (a slot past S), and a maximum over such pairs only as "does not count"
constexpr float kAbsent = -__builtin_huge_valf();
__device__ inline float present(float v) { return v == kAbsent ? -1.0f : v; }

// HALF: k-steps held in registers per lane (dim <= 2 * HALF)
template <int HALF>
__global__ void __launch_bounds__(64 * kWunschMaxWaves)
k_wunsch_topk(const WunschTask *__restrict__ tasks, const MatchUnit *__restrict__ units, const float *__restrict__ desc,
              const unsigned char *__restrict__ vmask, int dim, int S, int kcap, unsigned short *__restrict__ out_col,
              float *__restrict__ out_score) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int threads = (int)blockDim.x, stride = dim + kMatchPad, half = dim >> 1;
  float *sB = reinterpret_cast<float *>(smem);                                       // [32][stride], k permuted
  u64 *lists = reinterpret_cast<u64 *>(smem + sizeof(float) * kMatchTile * stride);  // [wave][slot][line, half]

  const MatchUnit unit = units[blockIdx.x];
  const WunschTask T = tasks[unit.task];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int line = unit.row0 + wave * kWunschTileLines + (r >> 3), s = r & 7;
  const bool line_ok = line < T.na, row_ok = line_ok && s < S;
  const unsigned m1 = line_ok ? vmask[T.la0 + line] : 0u;
  const bool valid1 = (m1 >> s) & 1u;
  u64 *my = lists + (size_t)wave * kcap * kListStride + (r >> 3) * 2 + h;

  float ra[HALF];  // this lane's k-steps of its point row; slots past S and lines past the image are zero rows
  load_row<HALF>(desc + (T.a0 + (row_ok ? (long long)line * S + s : 0)) * (long long)dim, dim, row_ok, h, ra);

  int cnt = 0;
  u64 thr = 0ull;
  for (int col0 = 0; col0 < T.nb; col0 += kWunschTileLines) {
    // 4 lines of image b as 32 slots
    stage_tile(sB, dim, threads, [&](int c, const float *&src) {
      const int bl = col0 + (c >> 3), bt = c & 7;
      src = desc + (T.b0 + (long long)bl * S + bt) * (long long)dim;
      return bl < T.nb && bt < S;
    });

    unsigned m2s[kWunschTileLines];  // validity bytes of the tile's lines (uniform), fetched under the MFMAs
#pragma unroll
    for (int jl = 0; jl < kWunschTileLines; ++jl) m2s[jl] = col0 + jl < T.nb ? vmask[T.lb0 + col0 + jl] : 0u;

    const f32x16 acc = mfma_tile<HALF>(reinterpret_cast<const float4 *>(sB + r * stride + h * half), ra, dim);

    // pooling: one neighbour line (4 registers) at a time
    float sc[kWunschTileLines];
#pragma unroll
    for (int jl = 0; jl < kWunschTileLines; ++jl) {
      const unsigned m2 = m2s[jl];
      // a real slot pair holds its score, or -1.0f where a sample is masked; a pair with a slot past S is ABSENT: it
      // holds -inf, which loses every wunsch_max (no score is -inf: the inputs are bounded), so that a real score below
      // -1.0f is not replaced by a padded slot's -1.0f.  A maximum over absent pairs only does not count (-1.0f).
      float p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = u + 4 * h;
        p[u] = (s < S && t < S) ? ((valid1 && ((m2 >> t) & 1u)) ? acc[4 * jl + u] : -1.0f) : kAbsent;
      }
      // a[s] = max over t, then the mean over s of the maxima that count
      float a = wunsch_max(wunsch_max(p[0], p[1]), wunsch_max(p[2], p[3]));
      a = present(wunsch_max(a, __shfl_xor(a, 32)));
      const float ls1 = wunsch_mean(sum8(wunsch_term(a)), cnt8(wunsch_counts(a)));
      // b[t] = max over s, then the mean over t
      int c2 = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p[u] = present(max8(p[u]));
        c2 += wunsch_counts(p[u]);
      }
      float s2 = (wunsch_term(p[0]) + wunsch_term(p[1])) + (wunsch_term(p[2]) + wunsch_term(p[3]));
      s2 = s2 + __shfl_xor(s2, 32);
      c2 += __shfl_xor(c2, 32);
      sc[jl] = wunsch_line_score(ls1, wunsch_mean(s2, c2));
    }
    // one lane of every 8 feeds the lists: half h takes the neighbour lines 2 h, 2 h + 1 of the tile, so both halves
    // insert at the same time
    if (s == 0 && line_ok) {
#pragma unroll 1
      for (int e = 0; e < 2; ++e) {
        const float score = e ? (h ? sc[3] : sc[1]) : (h ? sc[2] : sc[0]);
        const int col = col0 + 2 * h + e;
        if (col < T.nb) {
          const u64 key = match_key(score, (unsigned)col);
          if (key > thr) topk_insert<kListStride>(my, kcap, cnt, thr, key);
        }
      }
    }
  }

  // the lists of lanes r and r + 32 hold the line's columns: its kk best, best first
  const long long o = T.out0 + (long long)line * T.kk;
  merge_lists<kListStride>(h == 0 && s == 0 && line_ok, my, my + 1, cnt, T.kk, out_col + o, out_score + o);
}

// One group of kWunschNwGroup lanes per (task, line): lane `sub` takes the candidates sub, sub + 16, ...; it restates
// their S x S blocks with scalar fmaf in ascending k (the bits of the MFMA chain), runs both dynamic programs and keeps
// its best (value, position).  Positions are those of upstream's list: the candidates ascending in the key (slot kk - 1
// first), then the same candidates reversed; the first maximum wins, i.e. the smallest position among equal values.
template <int S>
__global__ void __launch_bounds__(256)
k_wunsch_nw(const WunschTask *__restrict__ tasks, const long long *__restrict__ prefix, int n_tasks, long long n_lines,
            const float *__restrict__ desc, const unsigned char *__restrict__ vmask, int dim,
            const unsigned short *__restrict__ col, const float *__restrict__ score, unsigned short *__restrict__ mcol,
            float *__restrict__ mscore) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long g = gid / kWunschNwGroup;
  const int sub = (int)(gid % kWunschNwGroup);
  const bool live = g < n_lines;  // (whole groups: 256 is a multiple of the group size)
  double best_v = -1.0e300;
  int best_pos = 0x7fffffff;
  WunschTask T = tasks[0];
  long long i = 0;
  if (live) {
    int lo = 0, hi = n_tasks;  // the task with prefix[t] <= g < prefix[t + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (prefix[mid] <= g) lo = mid;
      else hi = mid;
    }
    T = tasks[lo];
    i = g - prefix[lo];
    const unsigned m1 = vmask[T.la0 + i];
    const float *pa = desc + (T.a0 + i * S) * (long long)dim;
    for (int slot = sub; slot < T.kk; slot += kWunschNwGroup) {
      const long long j = col[T.out0 + i * T.kk + slot];
      if (j >= T.nb) continue;  // (cannot happen: kernel 1 fills every slot with a line of b)
      const unsigned m2 = vmask[T.lb0 + j];
      const float *pb = desc + (T.b0 + j * S) * (long long)dim;
      float P[S * S];
#pragma unroll
      for (int e = 0; e < S * S; ++e) P[e] = 0.0f;
      for (int k = 0; k < dim; k += 4) {
        float4 a[S], b[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          a[s] = *reinterpret_cast<const float4 *>(pa + (long long)s * dim + k);
          b[s] = *reinterpret_cast<const float4 *>(pb + (long long)s * dim + k);
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int t = 0; t < S; ++t) {
            float v = P[s * S + t];
            v = __builtin_fmaf(a[s].x, b[t].x, v);
            v = __builtin_fmaf(a[s].y, b[t].y, v);
            v = __builtin_fmaf(a[s].z, b[t].z, v);
            v = __builtin_fmaf(a[s].w, b[t].w, v);
            P[s * S + t] = v;
          }
      }
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t < S; ++t)
          if (!(((m1 >> s) & 1u) && ((m2 >> t) & 1u))) P[s * S + t] = -1.0f;
      const double vf = wunsch_nw<S>(P, S, false), vr = wunsch_nw<S>(P, S, true);
      const int pf = T.kk - 1 - slot, pr = pf + T.kk;
      if (vf > best_v || (vf == best_v && pf < best_pos)) { best_v = vf; best_pos = pf; }
      if (vr > best_v || (vr == best_v && pr < best_pos)) { best_v = vr; best_pos = pr; }
    }
  }
#pragma unroll
  for (int m = 1; m < kWunschNwGroup; m <<= 1) {
    const double ov = __shfl_xor(best_v, m);
    const int op = __shfl_xor(best_pos, m);
    if (ov > best_v || (ov == best_v && op < best_pos)) { best_v = ov; best_pos = op; }
  }
  if (live && sub == 0 && T.kk > 0) {
    const int slot = T.kk - 1 - (best_pos % T.kk);
    mcol[T.mout0 + i] = col[T.out0 + i * T.kk + slot];
    mscore[T.mout0 + i] = score[T.out0 + i * T.kk + slot];
  }
}

}  // namespace

void launch_wunsch_topk(hipStream_t st, int dim, int S, int kcap, int waves, const WunschTask *tasks,
                        const MatchUnit *units, int n_units, const float *desc, const unsigned char *vmask,
                        unsigned short *out_col, float *out_score) {
  if (n_units <= 0) return;
  const size_t lds = topk_lds_bytes(dim, kcap, waves, kListStride);
  const dim3 grid((unsigned)n_units), block(64u * (unsigned)waves);
#define LT_WUNSCH_LAUNCH(H)                                                                                        \
  do {                                                                                                             \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wunsch_topk<H>),                                   \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                               \
    hipLaunchKernelGGL((k_wunsch_topk<H>), grid, block, lds, st, tasks, units, desc, vmask, dim, S, kcap, out_col, \
                       out_score);                                                                                 \
  } while (0)
  if (dim <= 128) LT_WUNSCH_LAUNCH(64);
  else LT_WUNSCH_LAUNCH(128);
#undef LT_WUNSCH_LAUNCH
}

void launch_wunsch_nw(hipStream_t st, int dim, int S, const WunschTask *tasks, const long long *prefix, int n_tasks,
                      long long n_lines, const float *desc, const unsigned char *vmask, const unsigned short *col,
                      const float *score, unsigned short *mcol, float *mscore) {
  if (n_lines <= 0 || n_tasks <= 0) return;
  const long long threads = n_lines * kWunschNwGroup;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
#define LT_WUNSCH_NW(SS)                                                                                          \
  case SS:                                                                                                        \
    hipLaunchKernelGGL((k_wunsch_nw<SS>), grid, block, 0, st, tasks, prefix, n_tasks, n_lines, desc, vmask, dim, \
                       col, score, mcol, mscore);                                                                 \
    break
  switch (S) {
    LT_WUNSCH_NW(2);
    LT_WUNSCH_NW(3);
    LT_WUNSCH_NW(4);
    LT_WUNSCH_NW(5);
    LT_WUNSCH_NW(6);
    LT_WUNSCH_NW(7);
    LT_WUNSCH_NW(8);
    default: break;  // (rejected by the host before any launch)
  }
#undef LT_WUNSCH_NW
}

void launch_wunsch_mutual(hipStream_t st, const WunschTask *tasks, int n_pairs, unsigned short *mcol) {
  launch_mutual<WunschTask, &WunschTask::mout0>(st, tasks, n_pairs, 1, mcol);
}

}  // namespace lt
