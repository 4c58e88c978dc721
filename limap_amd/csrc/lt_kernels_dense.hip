// lt_kernels_dense.hip -- the dense-warp line matcher on the device ("Dense"): the samples of every line
// through the pair's warp (k_dense_warp), per (line of image 1, line of image 2) the two directions' weighted distance
// and overlap and their combination (k_dense_pairs: neither direction's (N, S, N) intermediate reaches memory, only the
// N1 x N2 dists do), and per line of image 1 the row minimum, the match flags and the compaction (k_dense_select, as
// a count pass and a fill pass around a prefix sum).  Every value is the expression of lt_dense.h, which the host
// restatement evaluates too.
//
// Tile layout of k_dense_pairs.  256 lanes own a 16 x 16 tile: lane t the entry (i0 + t / 16, j0 + t % 16).  LDS holds
// the warped samples of the tile's 16 + 16 lines sample-major ([k][16], x and y apart), so the 16 lanes that differ in j
// read 16 consecutive words in the 2 -> 1 loop and the 4 values of i in a wave 4 consecutive words (a broadcast each) in
// the 1 -> 2 loop: no bank conflict without padding.  At S = 64: 4 x 4 KB of samples, 256 B of flag words, 1 KB of line
// terms, 776 B of tables.

#include "lt_dense.h"

namespace lt {

namespace {

constexpr int kT = kDenseTile;
constexpr int kMaxS = kDenseMaxSamples;

__global__ void __launch_bounds__(256)
k_dense_warp(const DenseDir *__restrict__ dirs, int S, float thresh, const float *__restrict__ lines,
             const float *__restrict__ tab, float *__restrict__ wx, float *__restrict__ wy,
             unsigned char *__restrict__ wok) {
  const DenseDir D = dirs[blockIdx.x];
  const long long t = (long long)blockIdx.y * 256 + threadIdx.x;
  if (t >= (long long)D.n * S) return;
  const int k = (int)(t / D.n), l = (int)(t - (long long)k * D.n);
  const float4 ln = reinterpret_cast<const float4 *>(lines)[D.src0 + l];
  const float seg[4] = {ln.x, ln.y, ln.z, ln.w};
  float xs, ys, x, y;
  dense_sample(seg, tab[kDenseTabR + k], xs, ys);
  const bool ok = dense_warp_point(D.warp, D.cert, D.hw, D.ww, D.ax, D.ay, D.tw, D.th, thresh, xs, ys, x, y);
  const long long slot = D.smp0 + t;  // = smp0 + k * n + l
  wx[slot] = x;
  wy[slot] = y;
  wok[slot] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(256)
k_dense_pairs(const DenseTask *__restrict__ tasks, const DenseUnit *__restrict__ units, int S, float seg_th, float pix_th,
              const DenseLine *__restrict__ terms, const float *__restrict__ tab, const float *__restrict__ wx,
              const float *__restrict__ wy, const unsigned char *__restrict__ wok, float *__restrict__ dists,
              float *__restrict__ aux, long long total) {
  __shared__ float s1x[kMaxS * kT], s1y[kMaxS * kT], s2x[kMaxS * kT], s2y[kMaxS * kT];
  __shared__ unsigned long long m1[kT], m2[kT];
  __shared__ float L1[kT * 8], L2[kT * 8];
  __shared__ float s_ovl[kMaxS + 1], s_inv[kMaxS + 1];

  const DenseUnit U = units[blockIdx.x];
  const DenseTask T = tasks[U.task];
  const int tid = threadIdx.x;

  for (int idx = tid; idx < S * kT; idx += 256) {
    const int k = idx / kT, l = idx % kT;
    const int i = U.i0 + l, j = U.j0 + l;
    const bool in1 = i < T.n1, in2 = j < T.n2;
    const long long a = T.s12 + (long long)k * T.n1 + i, b = T.s21 + (long long)k * T.n2 + j;
    s1x[idx] = in1 ? wx[a] : 0.0f;
    s1y[idx] = in1 ? wy[a] : 0.0f;
    s2x[idx] = in2 ? wx[b] : 0.0f;
    s2y[idx] = in2 ? wy[b] : 0.0f;
  }
  if (tid < 2 * kT) {  // the flag word of a line: bit k = sample k's certainty passes
    const bool second = tid >= kT;
    const int l = tid % kT;
    const int line = (second ? U.j0 : U.i0) + l, n = second ? T.n2 : T.n1;
    unsigned long long m = 0ull;
    if (line < n) {
      const long long base = (second ? T.s21 : T.s12) + line;
      for (int k = 0; k < S; ++k) m |= (unsigned long long)(wok[base + (long long)k * n] != 0) << k;
    }
    (second ? m2 : m1)[l] = m;
  }
  {
    const bool second = tid >= kT * 8;
    const int idx = tid % (kT * 8), l = idx / 8;
    const int line = (second ? U.j0 : U.i0) + l, n = second ? T.n2 : T.n1;
    const float *src = reinterpret_cast<const float *>(terms + (second ? T.b0 : T.a0) + (second ? U.j0 : U.i0));
    (second ? L2 : L1)[idx] = line < n ? src[idx] : 0.0f;
  }
  if (tid <= S) {
    s_ovl[tid] = tab[kDenseTabOvl + tid];
    s_inv[tid] = tab[kDenseTabInv + tid];
  }
  __syncthreads();

  const int ti = tid / kT, tj = tid % kT;
  const int i = U.i0 + ti, j = U.j0 + tj;
  DenseLine A, B;  // line i of image 1, line j of image 2
  A.dx = L1[ti * 8 + 0]; A.dy = L1[ti * 8 + 1]; A.sp = L1[ti * 8 + 2]; A.ep = L1[ti * 8 + 3];
  A.lx = L1[ti * 8 + 4]; A.ly = L1[ti * 8 + 5]; A.lz = L1[ti * 8 + 6]; A.pad_ = 0.0f;
  B.dx = L2[tj * 8 + 0]; B.dy = L2[tj * 8 + 1]; B.sp = L2[tj * 8 + 2]; B.ep = L2[tj * 8 + 3];
  B.lx = L2[tj * 8 + 4]; B.ly = L2[tj * 8 + 5]; B.lz = L2[tj * 8 + 6]; B.pad_ = 0.0f;
  float d12, o12, d21, o21;
  dense_direction(s1x + ti, s1y + ti, kT, m1[ti], B, S, s_ovl, s_inv, seg_th, d12, o12);
  dense_direction(s2x + tj, s2y + tj, kT, m2[tj], A, S, s_ovl, s_inv, seg_th, d21, o21);
  if (i < T.n1 && j < T.n2) {
    const long long e = T.d0 + (long long)i * T.n2 + j;
    dists[e] = dense_combine(d12, o12, d21, o21, seg_th, pix_th);
    if (aux) {
      aux[e] = d12;
      aux[total + e] = o12;
      aux[2 * total + e] = d21;
      aux[3 * total + e] = o21;
    }
  }
}

__device__ inline float wave_min(float m) {
  for (int s = 32; s > 0; s >>= 1) {
    const float o = __shfl_xor(m, s);
    m = o < m ? o : m;
  }
  return m;
}

__global__ void __launch_bounds__(256)
k_dense_select(const DenseTask *__restrict__ tasks, int fill, int one_to_many, float pix_th,
               const float *__restrict__ dists, unsigned *__restrict__ cnt, const long long *__restrict__ off,
               int *__restrict__ out_line, unsigned short *__restrict__ out_col, float *__restrict__ out_score) {
  const DenseTask T = tasks[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= T.n1) return;  // (a whole wave)
  const float *row = dists + T.d0 + (long long)i * T.n2;
  float m = __builtin_huge_valf();
  if (!one_to_many) {
    for (int j = lane; j < T.n2; j += 64) {
      const float v = row[j];
      m = v < m ? v : m;
    }
    m = wave_min(m);
  }
  long long pos = fill ? off[T.r0 + i] : 0;
  unsigned n = 0;
  for (int j0 = 0; j0 < T.n2; j0 += 64) {
    const int j = j0 + lane;
    const float v = j < T.n2 ? row[j] : 0.0f;
    const bool hit = j < T.n2 && v <= pix_th && (one_to_many || v == m);
    const unsigned long long mask = __ballot(hit);
    if (fill && hit) {
      const long long p = pos + __popcll(mask & ((1ull << lane) - 1ull));
      out_line[p] = i;
      out_col[p] = (unsigned short)j;
      out_score[p] = v;
    }
    const int c = __popcll(mask);
    pos += c;
    n += (unsigned)c;
  }
  if (!fill && lane == 0) cnt[T.r0 + i] = n;
}

}  // namespace

void launch_dense_warp(hipStream_t st, const DenseDir *dirs, int n_dirs, int max_n, int S, float thresh,
                       const float *lines, const float *tab, float *wx, float *wy, unsigned char *wok) {
  if (n_dirs <= 0 || max_n <= 0) return;
  const unsigned chunks = (unsigned)(((long long)max_n * S + 255) / 256);
  hipLaunchKernelGGL(k_dense_warp, dim3((unsigned)n_dirs, chunks), dim3(256), 0, st, dirs, S, thresh, lines, tab, wx, wy,
                     wok);
}

void launch_dense_pairs(hipStream_t st, const DenseTask *tasks, const DenseUnit *units, int n_units, int S, float seg_th,
                        float pix_th, const DenseLine *terms, const float *tab, const float *wx, const float *wy,
                        const unsigned char *wok, float *dists, float *aux, long long total) {
  if (n_units <= 0) return;
  hipLaunchKernelGGL(k_dense_pairs, dim3((unsigned)n_units), dim3(256), 0, st, tasks, units, S, seg_th, pix_th, terms, tab,
                     wx, wy, wok, dists, aux, total);
}

void launch_dense_select(hipStream_t st, const DenseTask *tasks, int n_tasks, int max_n1, int fill, int one_to_many,
                         float pix_th, const float *dists, unsigned *cnt, const long long *off, int *out_line,
                         unsigned short *out_col, float *out_score) {
  if (n_tasks <= 0 || max_n1 <= 0) return;
  hipLaunchKernelGGL(k_dense_select, dim3((unsigned)n_tasks, (unsigned)((max_n1 + 3) / 4)), dim3(256), 0, st, tasks, fill,
                     one_to_many, pix_th, dists, cnt, off, out_line, out_col, out_score);
}

}  // namespace lt
