// lt_kernels_l23.hip -- 2D-3D line matching for localization on the device: every expression comes from
// lt_l23.h, which lt_l23.cpp compiles for the host twin too.
//   k_l23_cams     one lane per database or query camera: the Cam record
//   k_l23_recs     one lane per database segment (its 64-byte record) or task (the fundamental matrix query -> image)
//   k_l23_pairs    all_pairs.  One wave64 per (task, query line) walks the task's database lines in chunks of 64, one
//                  line per lane; the ballot of the test gives the chunk's survivors.  <false> counts them, <true>
//                  evaluates the test again (it is deterministic) and stores the rows at the unit's offset plus the
//                  popcount of the ballot below the lane: upstream's order without atomics and without a sort
//   k_l23_scan     one wave per query: a line's key is the first task with a survivor; lines in (key, id) order by a
//                  counting pass over the tasks; the exclusive scan of the lines' totals and of every line's units
//   k_l23_listed   listed modes: one lane per listed pair writes its keep flag
//   k_l23_filter   one wave per keyed line, lanes over its candidates in strides of 64; a skipped candidate is +inf; the
//                  minimum of (loss, track id) by a fixed xor tree of shuffles; lane 0 stores it
//   k_l23_compact  one wave per query drops the lines without a winner, in key order
// All stores are ordinary vector stores; there are no atomics, so nothing depends on the launch geometry or on timing.

#include "lt_devfn.h"
#include "lt_l23.h"

namespace lt {

namespace {

__global__ void __launch_bounds__(kL23Block) k_l23_cams(L23Dev d) {
  const long long i = (long long)blockIdx.x * kL23Block + threadIdx.x;
  if (i < d.n_db) {
    const double *c = d.db_cam11 + 11 * i;
    cam_build(c, c + 4, c + 8, &d.db_cam[i]);
  } else if (i < d.n_db + d.n_query) {
    const double *c = d.q_cam11 + 11 * (i - d.n_db);
    cam_build(c, c + 4, c + 8, &d.q_cam[i - d.n_db]);
  }
}

__global__ void __launch_bounds__(kL23Block) k_l23_recs(L23Dev d) {
  const long long i = (long long)blockIdx.x * kL23Block + threadIdx.x;
  if (i < d.n_dbseg) {
    const long long img = l23_find(d.db_seg_off, d.n_db, i);
    L23DbSeg r;
    l23_dbseg_build(d.db_cam[img], d.db_seg4 + 4 * i, &r);
    d.db_rec[i] = r;
  } else if (i < d.n_dbseg + d.n_task) {
    const long long t = i - d.n_dbseg;
    PairRec p;
    pair_build(d.q_cam[d.task_q[t]], d.db_cam[d.task_db[t]], &p);
    for (int k = 0; k < 9; ++k) d.task_F[9 * t + k] = p.F[k];
  }
}

template <bool FILL>
__global__ void __launch_bounds__(kL23Block) k_l23_pairs(L23Dev d) {
  const long long u = (long long)blockIdx.x * (kL23Block / 64) + (threadIdx.x >> 6);
  if (u >= d.n_units) return;  // wave-uniform
  const int lane = lane_id();
  const long long t = l23_find(d.unit_off, d.n_task, u);
  const long long i = u - d.unit_off[t];
  const int q = d.task_q[t], img = d.task_db[t];
  double s4[4], F[9];
  for (int k = 0; k < 4; ++k) s4[k] = d.q_seg4[4 * (d.q_seg_off[q] + i) + k];
  for (int k = 0; k < 9; ++k) F[k] = d.task_F[9 * t + k];
  const long long j0 = d.db_seg_off[img], nd = d.db_seg_off[img + 1] - j0;
  const long long base = FILL ? d.q_row0[q] + (long long)d.unit_pos[u] : 0;
  long long run = 0;
  for (long long c = 0; c < nd; c += 64) {
    const long long j = c + lane;
    bool ok = false;
    int track = -1;
    if (j < nd) {
      ok = l23_iou_test(d.cfg, s4, d.db_rec[j0 + j], F);
      if (ok) {  // the track id is loaded only to complete the test
        track = d.db_track[j0 + j];
        ok = track != -1;
      }
    }
    const unsigned long long b = __ballot(ok);
    if (FILL && ok) {
      const long long pos = base + run + __popcll(b & lanemask_lt());
      if (pos < d.rows_cap) reinterpret_cast<int2 *>(d.rows2)[pos] = make_int2((int)i, track);
    }
    run += __popcll(b);
  }
  if (!FILL && lane == 0) d.count[u] = (unsigned)run;
}

__global__ void __launch_bounds__(64) k_l23_scan(L23Dev d) {
  const long long q = blockIdx.x;
  const int lane = threadIdx.x;
  const long long t0 = d.task_off[q], K = d.task_off[q + 1] - t0;
  const long long s0 = d.q_seg_off[q], L = d.q_seg_off[q + 1] - s0;
  // a line's first task with a survivor and its total
  for (long long i = lane; i < L; i += 64) {
    long long f = K, tt = 0;
    for (long long k = 0; k < K; ++k) {
      const unsigned c = d.count[d.unit_off[t0 + k] + i];
      if (c && f == K) f = k;
      tt += c;
    }
    d.first[s0 + i] = (int)f;
    d.tot[s0 + i] = tt;
  }
  __syncthreads();
  // the keyed lines in (first task, line id) order
  long long nk = 0;
  for (long long k = 0; k < K; ++k)
    for (long long c = 0; c < L; c += 64) {
      const long long i = c + lane;
      const bool ok = i < L && d.first[s0 + i] == (int)k;
      const unsigned long long b = __ballot(ok);
      if (ok) d.kl_line[s0 + nk + __popcll(b & lanemask_lt())] = (int)i;
      nk += __popcll(b);
    }
  __syncthreads();
  // the exclusive scan of their totals
  long long run = 0;
  for (long long c = 0; c < nk; c += 64) {
    const long long p = c + lane;
    const long long v = p < nk ? d.tot[s0 + d.kl_line[s0 + p]] : 0;
    long long incl = v;
    for (int s = 1; s < 64; s <<= 1) {
      const long long o = __shfl_up(incl, s);
      if (lane >= s) incl += o;
    }
    if (p < nk) {
      d.kl_start[s0 + p] = run + incl - v;
      d.kl_cnt[s0 + p] = v;
    }
    run += __shfl(incl, 63);
  }
  __syncthreads();
  // every unit's first row: the line's units follow each other in task order
  for (long long p = lane; p < nk; p += 64) {
    const long long i = d.kl_line[s0 + p];
    long long pos = d.kl_start[s0 + p];
    for (long long k = 0; k < K; ++k) {
      const long long u = d.unit_off[t0 + k] + i;
      d.unit_pos[u] = (unsigned)pos;
      pos += d.count[u];
    }
  }
  if (lane == 0) {
    d.q_total[2 * q] = run;
    d.q_total[2 * q + 1] = nk;
  }
}

__global__ void __launch_bounds__(kL23Block) k_l23_listed(L23Dev d) {
  const long long idx = (long long)blockIdx.x * kL23Block + threadIdx.x;
  if (idx >= d.n_pairs) return;
  const long long t = l23_find(d.pair_off, d.n_task, idx);
  const int q = d.task_q[t], img = d.task_db[t];
  const long long i = d.q_seg_off[q] + d.pairs2[2 * idx], j = d.db_seg_off[img] + d.pairs2[2 * idx + 1];
  bool ok = true;
  if (d.cfg.mode == kL23ListedFiltered) ok = l23_iou_test(d.cfg, d.q_seg4 + 4 * i, d.db_rec[j], d.task_F + 9 * t);
  if (ok) ok = d.db_track[j] != -1;
  d.keep[idx] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kL23Block) k_l23_filter(L23Dev d) {
  const long long slot = (long long)blockIdx.x * (kL23Block / 64) + (threadIdx.x >> 6);
  if (slot >= d.n_qseg) return;  // wave-uniform
  const int lane = lane_id();
  const long long q = l23_find(d.q_seg_off, d.n_query, slot);
  const long long p = slot - d.q_seg_off[q];
  if (p >= d.q_total[2 * q + 1]) {
    if (lane == 0) d.win_track[slot] = -1;
    return;
  }
  const double *s4 = d.q_seg4 + 4 * (d.q_seg_off[q] + d.kl_line[slot]);
  const L2 ref{mk2(s4[0], s4[1]), mk2(s4[2], s4[3])};
  const Cam &cam = d.q_cam[q];
  const long long start = d.q_row0[q] + d.kl_start[slot], n = d.kl_cnt[slot];
  double best = kL23Inf;
  int best_t = 0x7FFFFFFF;
  for (long long c = lane; c < n; c += 64) {
    const int t = d.rows2[2 * (start + c) + 1];
    const double loss = l23_cand_loss(d.cfg, cam, ref, d.track6 + 6 * (long long)t);
    if (l23_better(loss, t, best, best_t)) {
      best = loss;
      best_t = t;
    }
  }
  for (int s = 32; s >= 1; s >>= 1) {
    const double lo = __shfl_xor(best, s);
    const int to = __shfl_xor(best_t, s);
    if (l23_better(lo, to, best, best_t)) {
      best = lo;
      best_t = to;
    }
  }
  if (lane == 0) {
    d.win_track[slot] = best < kL23Inf ? best_t : -1;
    d.win_loss[slot] = best;
  }
}

__global__ void __launch_bounds__(64) k_l23_compact(L23Dev d) {
  const long long q = blockIdx.x;
  const int lane = threadIdx.x;
  const long long s0 = d.q_seg_off[q], nk = d.q_total[2 * q + 1];
  long long run = 0;
  for (long long c = 0; c < nk; c += 64) {
    const long long p = c + lane;
    const bool ok = p < nk && d.win_track[s0 + p] >= 0;
    const unsigned long long b = __ballot(ok);
    if (ok) {
      const long long o = s0 + run + __popcll(b & lanemask_lt());
      reinterpret_cast<int2 *>(d.out_rows2)[o] = make_int2(d.kl_line[s0 + p], d.win_track[s0 + p]);
      d.out_loss[o] = d.win_loss[s0 + p];
    }
    run += __popcll(b);
  }
  if (lane == 0) d.out_cnt[q] = run;
}

unsigned blocks_of(long long n, long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_l23_build(hipStream_t st, const L23Dev &d) {
  if (d.n_db + d.n_query > 0)
    hipLaunchKernelGGL(k_l23_cams, dim3(blocks_of(d.n_db + d.n_query, kL23Block)), dim3(kL23Block), 0, st, d);
  if (d.n_dbseg + d.n_task > 0)
    hipLaunchKernelGGL(k_l23_recs, dim3(blocks_of(d.n_dbseg + d.n_task, kL23Block)), dim3(kL23Block), 0, st, d);
}

void launch_l23_count(hipStream_t st, const L23Dev &d) {
  if (d.n_units > 0)
    hipLaunchKernelGGL(k_l23_pairs<false>, dim3(blocks_of(d.n_units, kL23Block / 64)), dim3(kL23Block), 0, st, d);
}

void launch_l23_scan(hipStream_t st, const L23Dev &d) {
  if (d.n_query > 0) hipLaunchKernelGGL(k_l23_scan, dim3((unsigned)d.n_query), dim3(64), 0, st, d);
}

void launch_l23_fill(hipStream_t st, const L23Dev &d) {
  if (d.n_units > 0 && d.rows_cap > 0)
    hipLaunchKernelGGL(k_l23_pairs<true>, dim3(blocks_of(d.n_units, kL23Block / 64)), dim3(kL23Block), 0, st, d);
}

void launch_l23_listed(hipStream_t st, const L23Dev &d) {
  if (d.n_pairs > 0) hipLaunchKernelGGL(k_l23_listed, dim3(blocks_of(d.n_pairs, kL23Block)), dim3(kL23Block), 0, st, d);
}

void launch_l23_filter(hipStream_t st, const L23Dev &d) {
  if (d.n_qseg > 0)
    hipLaunchKernelGGL(k_l23_filter, dim3(blocks_of(d.n_qseg, kL23Block / 64)), dim3(kL23Block), 0, st, d);
  if (d.n_query > 0) hipLaunchKernelGGL(k_l23_compact, dim3((unsigned)d.n_query), dim3(64), 0, st, d);
}

}  // namespace lt
