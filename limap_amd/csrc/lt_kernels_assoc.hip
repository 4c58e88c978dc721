// lt_kernels_assoc.hip -- the global point-line association on the device: every expression comes from
// lt_assoc.h, which lt_assoc.cpp compiles for the host path too.  The status record carries a phase; a batch the host
// enqueues is the head of an attempt, a number of CG iterations and the tail of an attempt, and every kernel returns at
// once unless the record is in its phase, so the result does not depend on how the host cuts the batches.
//   head   k_as_linearize  one lane per R1 block and per association edge: residuals, rho', Jacobians by passes of four
//                          derivatives, and the edge's off-diagonal block rho' J_a^T J_b (after an accepted step only)
//          k_as_diag       one 16-lane group per point and line: the R1 sums (lane stride, xor tree), then lane 0 adds
//                          the unknown's edges in ascending edge order (after an accepted step only)
//          k_as_diag_vp    one wave64 per vanishing point: its ascending edge list in lane stride, then the xor tree
//          k_as_precond    one wave64 per chunk of 256 unknowns: the damped diagonal block, its inverse, x = 0, r = -g,
//                          z = p = M^-1 r, the chunk's part of r . z
//          k_as_cg_begin   one wave: r0 . z0, the zero-gradient end, a bad pivot
//   CG     k_as_matvec     one wave64 per chunk: Ap = A p per row -- the diagonal block, then the edges in ascending
//                          order -- and the chunk's part of p . Ap
//          k_as_alpha      one wave: p . Ap, the breakdown test, alpha
//          k_as_update     one wave64 per chunk: x, r, z and the chunk's part of r . z (x, r and A p are pairs of
//                          doubles: as_dd_acc of lt_assoc.h)
//          k_as_beta       one wave: r . z, the stop test, beta
//          k_as_dir        one lane per unknown: p = z + beta p
//   tail   k_as_backsub    one lane per unknown: the candidate parameters in the other set
//          k_as_cost       one wave64 per chunk of 256 blocks: the candidate cost and the model decrease's terms
//          k_as_decide     one wave: the chunks in lane stride, the xor tree, §27's decision (ba_decide_step)
// Kernel boundaries are the only synchronisation between workgroups: no cooperative launch, no grid barrier, no flag
// another workgroup waits for.  No floating-point atomics; no reduction depends on the grid.  All stores are ordinary
// vector stores of the lanes.

#include "lt_assoc.h"

namespace lt {

namespace {

__device__ __forceinline__ bool as_in_phase(const AsStatus *st, int phase) { return !st->lm.done && st->phase == phase; }

__global__ void __launch_bounds__(256) k_as_linearize(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsHead) || !st->lm.fresh) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < d.NB) as_item_lin_blk(d, st->lm.cur, i);
  else if (i < d.NB + d.NE) as_item_lin_edge(d, st->lm.cur, i - d.NB);
}

__global__ void __launch_bounds__(64) k_as_diag(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsHead) || !st->lm.fresh) return;
  const int lane = threadIdx.x % kAsWidth;
  const int u = blockIdx.x * (64 / kAsWidth) + threadIdx.x / kAsWidth;
  AsUnk un;
  un.b0 = un.nb = un.a0 = un.na = un.kind = un.nd = 0;
  if (u < d.NP + d.NL) un = d.unk[u];
  const bool live = un.nd != 0;
  if (!live) un.nb = 0;
  double part[kRfSums];
  as_struct_part(d, un, lane, part);
#pragma unroll
  for (int c = 0; c < kRfSums; ++c) part[c] = lm_group_sum<kAsWidth>(part[c]);
  if (live && lane == 0) as_item_diag_store(d, u, part);
}

__global__ void __launch_bounds__(kAsWave) k_as_diag_vp(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsHead) || !st->lm.fresh) return;
  const int u = d.NP + d.NL + blockIdx.x;
  const AsUnk un = d.unk[u];
  if (!un.nd) return;  // uniform over the wave
  double part[kRfSums];
  as_vp_part(d, un, threadIdx.x, part);
#pragma unroll
  for (int c = 0; c < kRfSums; ++c) part[c] = lm_group_sum<kAsWave>(part[c]);
  if (threadIdx.x == 0)
    for (int c = 0; c < kRfSums; ++c) d.D[(size_t)kRfSums * u + c] = part[c];
}

__global__ void __launch_bounds__(kAsWave) k_as_precond(AsDev d) {
  AsStatus *st = d.status;
  if (!as_in_phase(st, kAsHead)) return;
  const double mu = st->lm.mu;
  const int base = blockIdx.x * kAsChunk;
  double rz = 0.0, flag = 0.0;
  bool bad = false;
  for (int i = threadIdx.x; i < kAsChunk && base + i < d.NU; i += kAsWave) {
    const int u = base + i;
    bool ok = true, nz = false;
    as_item_damp(d, u, mu);
    rz = rz + as_item_cg_start(d, u, &ok, &nz);
    if (nz) flag = 1.0;
    bad = bad || !ok;
  }
  rz = lm_group_sum<kAsWave>(rz);
  flag = lm_group_sum<kAsWave>(flag);
  if (bad) st->lm.bad = 1;
  if (threadIdx.x == 0) {
    d.chunk[blockIdx.x] = rz;
    d.chunk[d.n_uchunks + blockIdx.x] = flag;
  }
}

__global__ void __launch_bounds__(kAsWave) k_as_cg_begin(AsDev d) {
  AsStatus st = *d.status;
  if (st.lm.done || st.phase != kAsHead) return;
  double rz, flag;
  lm_totals(d.chunk, d.n_uchunks, d.n_uchunks, &rz, &flag);
  as_decide_begin(st, rz, flag != 0.0);
  if (threadIdx.x == 0) *d.status = st;
}

__global__ void __launch_bounds__(kAsWave) k_as_matvec(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsCg)) return;
  const int base = blockIdx.x * kAsChunk;
  double pap = 0.0;
  for (int i = threadIdx.x; i < kAsChunk && base + i < d.NU; i += kAsWave) pap = pap + as_item_matvec(d, base + i);
  pap = lm_group_sum<kAsWave>(pap);
  if (threadIdx.x == 0) d.chunk[blockIdx.x] = pap;
}

__global__ void __launch_bounds__(kAsWave) k_as_alpha(AsDev d) {
  AsStatus st = *d.status;
  if (st.lm.done || st.phase != kAsCg) return;
  double pap, unused;
  lm_totals(d.chunk, d.n_uchunks, 0, &pap, &unused);
  as_decide_alpha(st, pap);
  if (threadIdx.x == 0) *d.status = st;
}

__global__ void __launch_bounds__(kAsWave) k_as_update(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsCg)) return;
  const double alpha = st->alpha;
  const int base = blockIdx.x * kAsChunk;
  double rz = 0.0;
  for (int i = threadIdx.x; i < kAsChunk && base + i < d.NU; i += kAsWave) rz = rz + as_item_update(d, base + i, alpha);
  rz = lm_group_sum<kAsWave>(rz);
  if (threadIdx.x == 0) d.chunk[blockIdx.x] = rz;
}

__global__ void __launch_bounds__(kAsWave) k_as_beta(AsDev d) {
  AsStatus st = *d.status;
  if (st.lm.done || st.phase != kAsCg) return;
  double rz, unused;
  lm_totals(d.chunk, d.n_uchunks, 0, &rz, &unused);
  as_decide_beta(st, rz);
  if (threadIdx.x == 0) *d.status = st;
}

__global__ void __launch_bounds__(256) k_as_dir(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsCg)) return;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u < d.NU) as_item_dir(d, u, st->beta);
}

__global__ void __launch_bounds__(256) k_as_backsub(AsDev d) {
  const AsStatus *st = d.status;
  if (!as_in_phase(st, kAsTail) || st->lm.bad) return;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u < d.NU) as_item_backsub(d, st->lm.cur, u);
}

// mode 0: the cost at the initial point (set 0; the status record is not read); 1: the candidate of an attempt
__global__ void __launch_bounds__(kAsWave) k_as_cost(AsDev d, int mode) {
  int set = 0;
  if (mode) {
    const AsStatus *st = d.status;
    if (!as_in_phase(st, kAsTail) || st->lm.bad) return;
    set = 1 - st->lm.cur;
  }
  double cost, md;
  lm_chunk_sums(d.NB + d.NE, [&](int i, double *a, double *b) {
    double c, m;
    as_item_cost(d, set, i, mode != 0, &c, &m);
    *a = *a + c;
    *b = *b + m;
  }, &cost, &md);
  if (threadIdx.x == 0) {
    d.chunk[blockIdx.x] = cost;
    d.chunk[d.n_chunks + blockIdx.x] = md;
  }
}

__global__ void __launch_bounds__(kAsWave) k_as_decide(AsDev d, int mode) {
  AsStatus st = *d.status;
  if (mode && (st.lm.done || st.phase != kAsTail)) return;
  double cost, md;
  lm_totals(d.chunk, d.n_chunks, d.n_chunks, &cost, &md);
  if (mode) ba_decide_step(st.lm, cost, md);
  else ba_decide_init(st.lm, cost);
  st.phase = kAsHead;
  if (threadIdx.x == 0) *d.status = st;
}

}  // namespace

void launch_as_init(hipStream_t s, const AsDev &d) {
  hipLaunchKernelGGL(k_as_cost, dim3((unsigned)d.n_chunks), dim3(kAsWave), 0, s, d, 0);
  hipLaunchKernelGGL(k_as_decide, dim3(1), dim3(kAsWave), 0, s, d, 0);
}

void launch_as_attempt(hipStream_t s, const AsDev &d, int cg_batch, hipEvent_t *ev) {
  int e = 0;
  auto mark = [&]() {
    if (ev) (void)hipEventRecord(ev[e++], s);
  };
  const dim3 wave(kAsWave), uch((unsigned)d.n_uchunks), per_u(lm_blocks_of(d.NU, 256));
  mark();
  hipLaunchKernelGGL(k_as_linearize, dim3(lm_blocks_of((long long)d.NB + d.NE, 256)), dim3(256), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_as_diag, dim3(lm_blocks_of((long long)d.NP + d.NL, 64 / kAsWidth)), dim3(64), 0, s, d);
  mark();
  if (d.NV > 0) hipLaunchKernelGGL(k_as_diag_vp, dim3((unsigned)d.NV), wave, 0, s, d);
  mark();
  hipLaunchKernelGGL(k_as_precond, uch, wave, 0, s, d);
  mark();
  hipLaunchKernelGGL(k_as_cg_begin, dim3(1), wave, 0, s, d);
  mark();
  for (int k = 0; k < cg_batch; ++k) {
    hipLaunchKernelGGL(k_as_matvec, uch, wave, 0, s, d);
    mark();
    hipLaunchKernelGGL(k_as_alpha, dim3(1), wave, 0, s, d);
    mark();
    hipLaunchKernelGGL(k_as_update, uch, wave, 0, s, d);
    mark();
    hipLaunchKernelGGL(k_as_beta, dim3(1), wave, 0, s, d);
    mark();
    hipLaunchKernelGGL(k_as_dir, per_u, dim3(256), 0, s, d);
    mark();
  }
  hipLaunchKernelGGL(k_as_backsub, per_u, dim3(256), 0, s, d);
  mark();
  hipLaunchKernelGGL(k_as_cost, dim3((unsigned)d.n_chunks), wave, 0, s, d, 1);
  mark();
  hipLaunchKernelGGL(k_as_decide, dim3(1), wave, 0, s, d, 1);
  mark();
}

}  // namespace lt
