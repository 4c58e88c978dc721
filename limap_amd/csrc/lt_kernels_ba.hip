// lt_kernels_ba.hip -- the bundle adjustment with free poses, points and lines on the device: every
// expression comes from lt_ba.h, which lt_ba.cpp compiles for the host path too.  One attempt of the Levenberg-Marquardt
// loop is the sequence
//   k_ba_linearize  one lane per residual block: r, rho', J_cam (2 x 6), J_struct (2 x 3 / 2 x 4) into the SoA table, by
//                   passes of three or four derivatives (after an accepted step only)
//   k_ba_blocks     one 16-lane group per structure track: V_s and b_s (lane stride, then the xor tree), then the W of
//                   its (track, image) pairs, a lane per pair (after an accepted step only)
//   k_ba_images     one wave64 per image: U_c and g_c from the image's ascending block list (lane stride, xor tree)
//   k_ba_damp       one lane per structure: V_s^{-1} of the damped block and Y = W V_s^{-1} of its pairs
//   k_ba_schur      one wave64 per image pair (i, j <= i): lane e < 36 owns one entry of the 6 x 6 block S_ij and walks
//                   the pair's couple list in ascending structure order; six more lanes of a diagonal block own the
//                   right-hand side.  No LDS, no barrier: no two lanes share an entry
//   k_ba_chol       one workgroup: the defined Cholesky factorisation column by column, every lane its rows' sums in
//                   ascending k; forward substitution by columns (ascending k per row); back substitution by one wave,
//                   its lanes multiplying 64 entries at a time and all of them subtracting the products in ascending k
//   k_ba_backsub    one lane per structure and per image: ds, dc and the candidate parameters in the other set
//   k_ba_cost       one wave64 per chunk of 256 blocks: the candidate cost and the model decrease's terms
//   k_ba_decide     one wave: the chunks in lane stride, the xor tree, the ratio test, the radius, the status record
// With constant poses the tracks separate: k_ba_point_lm runs the whole loop of a point track in its 16-lane group, as
// k_refine_lm does for a line track.
// No floating-point atomics; no reduction depends on the grid.  A kernel returns at once when the solve has ended or,
// past k_ba_damp, when the attempt's factorisation has failed.  All stores are ordinary vector stores of the lanes.

#include "lt_ba.h"

namespace lt {

namespace {

__global__ void __launch_bounds__(256) k_ba_linearize(BaDev d) {
  const BaStatus *st = d.status;
  if (st->done || !st->fresh) return;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < d.NB) ba_item_linearise(d, st->cur, b);
}

__global__ void __launch_bounds__(64) k_ba_blocks(BaDev d) {
  const BaStatus *st = d.status;
  if (st->done || !st->fresh) return;
  const int lane = threadIdx.x % kBaWidth;
  const int s = blockIdx.x * (64 / kBaWidth) + threadIdx.x / kBaWidth;
  const bool live = s < d.NS && !d.st[s].constant;
  BaStruct rec;
  rec.b0 = rec.nb = rec.p0 = rec.np = rec.kind = rec.constant = 0;
  if (live) rec = d.st[s];
  double part[kRfSums];
  ba_struct_part(d, rec, lane, part);
#pragma unroll
  for (int c = 0; c < kRfSums; ++c) part[c] = lm_group_sum<kBaWidth>(part[c]);
  if (live && lane == 0) {
    for (int c = 0; c < 10; ++c) d.V[(size_t)10 * s + c] = part[c];
    for (int c = 0; c < 4; ++c) d.bs[(size_t)4 * s + c] = part[10 + c];
  }
  if (live)
    for (int q = rec.p0 + lane; q < rec.p0 + rec.np; q += kBaWidth) ba_pair_W(d, q);
}

__global__ void __launch_bounds__(kBaWave) k_ba_images(BaDev d) {
  const BaStatus *st = d.status;
  if (st->done || !st->fresh) return;
  const int c = blockIdx.x;
  double part[kLcSums];
  ba_cam_part(d, c, threadIdx.x, part);
#pragma unroll
  for (int x = 0; x < kLcSums; ++x) part[x] = lm_group_sum<kBaWave>(part[x]);
  if (threadIdx.x == 0) {
    for (int x = 0; x < 21; ++x) d.U[(size_t)21 * c + x] = part[x];
    for (int x = 0; x < 6; ++x) d.g[(size_t)6 * c + x] = part[21 + x];
  }
}

__global__ void __launch_bounds__(256) k_ba_damp(BaDev d) {
  BaStatus *st = d.status;
  if (st->done) return;
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < d.NS && !ba_item_vinv(d, s, st->mu)) st->bad = 1;
}

__global__ void __launch_bounds__(kBaWave) k_ba_schur(BaDev d) {
  const BaStatus *st = d.status;
  if (st->done || st->bad) return;
  const int j = blockIdx.x, i = blockIdx.y, e = threadIdx.x;
  if (j <= i && e < 42) ba_item_schur(d, i, j, e, st->mu);
}

__global__ void __launch_bounds__(kBaCholThreads) k_ba_chol(BaDev d) {
  __shared__ double Lj[6 * kBaMaxImages];
  __shared__ double xs[6 * kBaMaxImages];
  __shared__ double diag;
  __shared__ int sbad;
  BaStatus *st = d.status;
  const int done = st->done, bad = st->bad, fresh = st->fresh;
  if (done || bad) return;
  const int tid = threadIdx.x, n = d.n;
  if (fresh) {  // g == 0 over all unknowns: the solve ends before the iteration counts
    int nz = 0;
    for (int i = tid; i < n; i += kBaCholThreads) nz |= d.g[i] != 0.0;
    for (int s = tid; s < d.NS; s += kBaCholThreads) {
      const BaStruct rec = d.st[s];
      if (rec.constant) continue;
      for (int l = 0; l < (rec.kind ? 4 : 3); ++l) nz |= d.bs[(size_t)4 * s + l] != 0.0;
    }
    if (!__syncthreads_or(nz)) {
      if (tid == 0) { st->code = kRfZeroGrad; st->done = 1; }
      return;
    }
  }
  double *LT = d.LT;
  for (int j = 0; j < n; ++j) {
    for (int k = tid; k < j; k += kBaCholThreads) Lj[k] = LT[(size_t)k * n + j];
    __syncthreads();
    // every row i >= j has a lane of its own (6 C <= kBaCholThreads)
    const int i = j + tid;
    double sum = 0.0;
    if (i < n) {
      double s = d.S[(size_t)i * n + j];
      int k = 0;
      for (; k + 16 <= j; k += 16) {  // sixteen loads in flight, then their sixteen steps of the chain in ascending k
        double a[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) a[u] = LT[(size_t)(k + u) * n + i];
#pragma unroll
        for (int u = 0; u < 16; ++u) s = s - a[u] * Lj[k + u];
      }
      for (; k < j; ++k) s = s - LT[(size_t)k * n + i] * Lj[k];
      sum = s;
    }
    if (tid == 0) {
      const bool ok = lm_pivot_ok(sum);
      sbad = ok ? 0 : 1;
      diag = ok ? sqrt(sum) : 1.0;
      if (ok) LT[(size_t)j * n + j] = diag;
    }
    __syncthreads();
    if (sbad) {
      if (tid == 0) st->bad = 1;
      return;
    }
    const double dd = diag;
    if (i < n && i != j) LT[(size_t)j * n + i] = sum / dd;
    __syncthreads();
  }
  // forward substitution by columns: row i = tid meets its k in ascending order
  double acc = tid < n ? d.rhs[tid] : 0.0;
  for (int k = 0; k < n; ++k) {
    if (tid == k) xs[k] = acc / LT[(size_t)k * n + k];
    __syncthreads();
    if (tid > k && tid < n) acc = acc - LT[(size_t)k * n + tid] * xs[k];
  }
  __syncthreads();
  // back substitution: x_i = (y_i - sum_{k > i} L_ki x_k) / L_ii in ascending k.  The chain is serial; the first wave
  // walks it, its lanes multiplying 64 entries at a time and every lane subtracting the products in ascending k
  if (tid < kBaWave) {
    for (int i = n - 1; i >= 0; --i) {
      double s = xs[i];
      const double *row = LT + (size_t)i * n;
      for (int kb = i + 1; kb < n; kb += kBaWave) {
        const int k = kb + tid;
        const double prod = k < n ? row[k] * xs[k] : 0.0;
        // (a lane past the row's end holds +0.0, and s - 0.0 is s: every chunk subtracts 64 values, lane index a constant)
#pragma unroll
        for (int m = 0; m < kBaWave; ++m) s = s - __shfl(prod, m, kBaWave);
      }
      s = s / row[i];
      if (tid == 0) xs[i] = s;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += kBaCholThreads) d.dc[i] = xs[i];
}

__global__ void __launch_bounds__(256) k_ba_backsub(BaDev d) {
  const BaStatus *st = d.status;
  if (st->done || st->bad) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < d.NS) ba_item_backsub_struct(d, st->cur, e);
  else if (e < d.NS + d.C) ba_item_backsub_cam(d, st->cur, e - d.NS);
}

// mode 0: the cost at the initial point (set 0; the status record is not read); 1: the candidate of an attempt
__global__ void __launch_bounds__(kBaWave) k_ba_cost(BaDev d, int mode) {
  int set = 0;
  if (mode) {
    const BaStatus *st = d.status;
    if (st->done || st->bad) return;
    set = 1 - st->cur;
  }
  double cost, md;
  lm_chunk_sums(d.NB, [&](int i, double *a, double *b) {
    double c, m;
    ba_item_cost(d, set, i, mode != 0, &c, &m);
    *a = *a + c;
    *b = *b + m;
  }, &cost, &md);
  if (threadIdx.x == 0) {
    d.chunk[blockIdx.x] = cost;
    d.chunk[d.n_chunks + blockIdx.x] = md;
  }
}

__global__ void __launch_bounds__(kBaWave) k_ba_decide(BaDev d, int mode) {
  BaStatus st = *d.status;
  if (mode && st.done) return;
  double cost, md;
  lm_totals(d.chunk, d.n_chunks, d.n_chunks, &cost, &md);
  if (mode) ba_decide_step(st, cost, md);
  else ba_decide_init(st, cost);
  if (threadIdx.x == 0) *d.status = st;
}

// constant poses: the whole loop of a point track by its 16-lane group (§19's k_refine_lm with three unknowns).  The
// group is the kernel's own; its host twin is BaPointGroup over LmHostLanes.  With BaPointGroup over the wave's lanes
// the kernel keeps its registers and is 10 % slower
struct PointGroup {
  const BaDev &d;
  const BaStruct &st;
  int lane;
  __device__ __forceinline__ double cost(const double p[3]) const {
    return 0.5 * lm_group_sum<kBaWidth>(ba_point_cost_part(d, st, lane, p));
  }
  __device__ __forceinline__ void linearise(const double p[3], double acc[kRfSums]) const {
    ba_point_lin_part(d, st, lane, p, acc);
#pragma unroll
    for (int c = 0; c < kRfSums; ++c) acc[c] = lm_group_sum<kBaWidth>(acc[c]);
  }
};

__global__ void __launch_bounds__(64) k_ba_point_lm(BaDev d, int max_iter, BaPtOut *__restrict__ out) {
  const int lane = threadIdx.x % kBaWidth;
  const int s = blockIdx.x * (64 / kBaWidth) + threadIdx.x / kBaWidth;
  const bool live = s < d.NS;
  BaStruct rec;
  rec.b0 = rec.nb = rec.p0 = rec.np = rec.kind = 0;
  rec.constant = 1;  // a group past the end runs the constant branch: no loop, uniform shuffles
  if (live) rec = d.st[s];
  double p[3] = {0.0, 0.0, 0.0}, F0, F1;
  int it, code;
  if (live)
    for (int c = 0; c < 3; ++c) p[c] = d.sp[(size_t)6 * s + c];
  PointGroup grp{d, rec, lane};
  ba_point_lm(grp, rec.constant != 0, max_iter, p, &F0, &F1, &it, &code);
  if (live && lane == 0) {
    for (int c = 0; c < 3; ++c) out[s].p[c] = p[c];
    out[s].cost0 = F0;
    out[s].cost1 = F1;
    out[s].iters = it;
    out[s].code = code;
  }
}

}  // namespace

void launch_ba_init(hipStream_t s, const BaDev &d) {
  hipLaunchKernelGGL(k_ba_cost, dim3((unsigned)d.n_chunks), dim3(kBaWave), 0, s, d, 0);
  hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(kBaWave), 0, s, d, 0);
}

void launch_ba_attempt(hipStream_t s, const BaDev &d, hipEvent_t *ev) {
  int e = 0;
  auto mark = [&]() {
    if (ev) (void)hipEventRecord(ev[e++], s);
  };
  mark();
  hipLaunchKernelGGL(k_ba_linearize, dim3(lm_blocks_of(d.NB, 256)), dim3(256), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_blocks, dim3(lm_blocks_of(d.NS, 64 / kBaWidth)), dim3(64), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_images, dim3((unsigned)d.C), dim3(kBaWave), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_damp, dim3(lm_blocks_of(d.NS, 256)), dim3(256), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_schur, dim3((unsigned)d.C, (unsigned)d.C), dim3(kBaWave), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_chol, dim3(1), dim3(kBaCholThreads), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_backsub, dim3(lm_blocks_of((long long)d.NS + d.C, 256)), dim3(256), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_ba_cost, dim3((unsigned)d.n_chunks), dim3(kBaWave), 0, s, d, 1);
  mark();
  hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(kBaWave), 0, s, d, 1);
  mark();
}

void launch_ba_points(hipStream_t s, const BaDev &d, int max_iter, BaPtOut *out) {
  if (d.NS <= 0) return;
  hipLaunchKernelGGL(k_ba_point_lm, dim3(lm_blocks_of(d.NS, 64 / kBaWidth)), dim3(64), 0, s, d, max_iter, out);
}

}  // namespace lt
