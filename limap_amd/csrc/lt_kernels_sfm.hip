// lt_kernels_sfm.hip -- device side of the visual neighbours (limap.pointsfm SfmModel::GetMax*Images).
//   k_sfm_pairs     one lane per instance slot (a pair of elements of one point track): the 64-bit key
//                   min(i, j) << 48 | max(i, j) << 32 | angle bits.  Slots, not points: a landmark track of 5 000
//                   images is 12.5 M slots spread over the grid, not one lane's loop
//   (sort)          launch_bpt_sort_keys of lt_kernels_bpt.hip over the keys
//   k_sfm_segments  one lane per sorted slot: the head of a run of equal (i, j) finds the run's end by binary search and
//                   writes one SfmPair (shared = run length, angle = the percentile element of the run); counted output,
//                   one atomic per wave
//   k_sfm_partners  per record: count, then fill, the partner lists of its two images
//   k_sfm_scan      exclusive sums of per-image counts (one workgroup)
//   k_sfm_select    one wave64 per image: gate by angle, score, and the rank of every kept partner under the total order
//                   (score descending, index ascending); the partners of rank < num_images are the neighbours
//   k_sfm_compact   the neighbours of all images into one dense array
// Atomics only add integers to counters and cursors: where a record or a list entry lands depends on the order in
// which they arrive, what is computed from them does not (every consumer either counts or ranks by a total order).

#include "lt_sfm.h"

namespace lt {

namespace {

inline unsigned grid_of(long long n) { return (unsigned)((n + kSfmBlock - 1) / kSfmBlock); }

__global__ void __launch_bounds__(kSfmBlock) k_sfm_pairs(long long n_slots, long long n_pts,
                                                         const long long *__restrict__ pair_off,
                                                         const long long *__restrict__ track_off,
                                                         const int *__restrict__ track_img,
                                                         const double *__restrict__ centres,
                                                         const float *__restrict__ xyz,
                                                         unsigned long long *__restrict__ keys) {
  const long long e = (long long)blockIdx.x * kSfmBlock + threadIdx.x;
  if (e >= n_slots) return;
  keys[e] = sfm_slot_key(e, n_pts, pair_off, track_off, track_img, centres, xyz);
}

__global__ void __launch_bounds__(kSfmBlock) k_sfm_segments(long long n_slots,
                                                            const unsigned long long *__restrict__ keys,
                                                            SfmPair *__restrict__ out, unsigned long long capacity,
                                                            unsigned long long *__restrict__ counter) {
  const long long s = (long long)blockIdx.x * kSfmBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  bool head = false;
  SfmPair rec{0u, 0u, 0u, 0u};
  if (s < n_slots) {
    const unsigned top = (unsigned)(keys[s] >> 32);
    head = top != 0xffffffffu && (s == 0 || (unsigned)(keys[s - 1] >> 32) != top);
    if (head) {
      long long lo = s, hi = n_slots;  // the run ends at the first slot whose upper half is greater
      while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if ((unsigned)(keys[mid] >> 32) <= top) lo = mid; else hi = mid;
      }
      const long long n = hi - s;
      rec.ij = top;
      rec.shared = (unsigned)n;
      rec.angle_bits = (unsigned)keys[s + sfm_percentile_index(n)];
    }
  }
  // (no lane has left: the ballot and the shuffle see the whole wave)
  const unsigned long long heads = __ballot(head);
  if (heads == 0ull) return;
  const int leader = __ffsll((long long)heads) - 1;
  unsigned long long base = 0ull;
  if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(heads));
  base = __shfl(base, leader);
  if (head) {
    const unsigned long long pos = base + (unsigned long long)__popcll(heads & ((1ull << lane) - 1ull));
    if (pos < capacity) out[pos] = rec;
  }
}

// adds one to ctr[img] for every active lane and returns the value the lane's own add saw.  Records leave
// k_sfm_segments in key order wave by wave, so the lanes of a wave mostly name one or two images on the i side: the
// first two distinct images take one atomic each for all their lanes, what is left takes one per lane.
__device__ __forceinline__ unsigned sfm_wave_add(unsigned *ctr, unsigned img, bool active, int lane) {
  unsigned pos = 0u;
  unsigned long long todo = __ballot(active);
  for (int r = 0; r < 2 && todo != 0ull; ++r) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned v = __shfl(img, leader);
    const unsigned long long same = __ballot(active && img == v) & todo;
    unsigned base = 0u;
    if (lane == leader) base = atomicAdd(&ctr[v], (unsigned)__popcll(same));
    base = __shfl(base, leader);
    if ((same >> lane) & 1ull) pos = base + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) pos = atomicAdd(&ctr[img], 1u);
  return pos;
}

template <int FILL>
__global__ void __launch_bounds__(kSfmBlock) k_sfm_partners(long long n_pairs, const SfmPair *__restrict__ pairs,
                                                            unsigned *__restrict__ cnt,
                                                            const long long *__restrict__ off,
                                                            unsigned *__restrict__ part) {
  const long long r = (long long)blockIdx.x * kSfmBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool active = r < n_pairs;
  const unsigned ij = active ? pairs[r].ij : 0u;
  const unsigned i = ij >> 16, j = ij & 0xffffu;
  const unsigned pi = sfm_wave_add(cnt, i, active, lane);
  const unsigned pj = sfm_wave_add(cnt, j, active, lane);
  if (FILL && active) {
    part[off[i] + pi] = (unsigned)r;
    part[off[j] + pj] = (unsigned)r;
  }
}

__global__ void __launch_bounds__(kSfmScanBlock) k_sfm_scan(int n, const unsigned *__restrict__ cnt,
                                                            long long *__restrict__ off) {
  __shared__ long long s_sum[kSfmScanBlock];
  const int t = (int)threadIdx.x;
  const int per = (n + kSfmScanBlock - 1) / kSfmScanBlock;
  const int k0 = t * per, k1 = k0 + per < n ? k0 + per : n;
  long long mine = 0;
  for (int k = k0; k < k1; ++k) mine += (long long)cnt[k];
  s_sum[t] = mine;
  __syncthreads();
  for (int d = 1; d < kSfmScanBlock; d <<= 1) {
    const long long add = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  long long run = s_sum[t] - mine;  // the sum of the lanes before this one
  for (int k = k0; k < k1; ++k) {
    off[k] = run;
    run += (long long)cnt[k];
  }
  if (t == kSfmScanBlock - 1) off[n] = s_sum[t];
}

__global__ void __launch_bounds__(64) k_sfm_select(const long long *__restrict__ off, unsigned *part, double *score,
                                                   const SfmPair *__restrict__ pairs, const int *__restrict__ n_pts,
                                                   int kind, float min_angle, long long num_images,
                                                   unsigned *__restrict__ nb, unsigned *__restrict__ nb_cnt) {
  __shared__ double s_score[64];
  __shared__ unsigned s_idx[64];
  const unsigned m = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const long long o = off[m], n = off[m + 1] - o;
  const int n_m = n_pts[m];
  // gate and score of every partner, once.  A partner the gate drops carries bit 31 of its index (indices take 16
  // bits); the score cannot mark it: a track that names its images more than once makes an IoU negative or infinite
  int kept = 0;
  for (long long k = lane; k < n; k += 64) {
    const SfmPair p = pairs[part[o + k]];
    const unsigned i = p.ij >> 16, j = p.ij & 0xffffu;
    const unsigned q = i == m ? j : i;
    const bool keep = sfm_from_bits32(p.angle_bits) >= min_angle;
    score[o + k] = sfm_score(kind, p.shared, n_m, n_pts[q]);
    part[o + k] = keep ? q : (q | kSfmDropped);
    kept += keep ? 1 : 0;
  }
  for (int d = 32; d > 0; d >>= 1) kept += __shfl_xor(kept, d);
  __threadfence_block();
  __syncthreads();
  // rounds of 64 owners; every round passes over all partners in tiles of 64 through LDS and counts, per owner, the
  // kept partners that come before it.  The order is total, so the ranks of the kept partners are 0 .. kept - 1
  for (long long ob = 0; ob < n; ob += 64) {
    const bool own = ob + lane < n;
    const double sc = own ? score[o + ob + lane] : 0.0;
    const unsigned ix = own ? part[o + ob + lane] : kSfmDropped;
    long long rank = 0;
    for (long long tb = 0; tb < n; tb += 64) {
      __syncthreads();
      const bool has = tb + lane < n;
      s_score[lane] = has ? score[o + tb + lane] : 0.0;
      s_idx[lane] = has ? part[o + tb + lane] : kSfmDropped;
      __syncthreads();
      const int tn = n - tb < 64 ? (int)(n - tb) : 64;
      for (int u = 0; u < tn; ++u)
        rank += ((s_idx[u] & kSfmDropped) == 0u && sfm_better(s_score[u], s_idx[u], sc, ix)) ? 1 : 0;
    }
    if ((ix & kSfmDropped) == 0u && rank < num_images) nb[o + rank] = ix;
  }
  if (lane == 0) nb_cnt[m] = (unsigned)((long long)kept < num_images ? (long long)kept : num_images);
}

__global__ void __launch_bounds__(64) k_sfm_compact(const long long *__restrict__ off, const unsigned *__restrict__ nb,
                                                    const unsigned *__restrict__ nb_cnt,
                                                    const long long *__restrict__ nb_off, int *__restrict__ dense) {
  const unsigned m = blockIdx.x;
  const long long src = off[m], dst = nb_off[m];
  const unsigned n = nb_cnt[m];
  for (unsigned k = threadIdx.x; k < n; k += 64u) dense[dst + k] = (int)nb[src + k];
}

}  // namespace

void launch_sfm_pairs(hipStream_t st, long long n_slots, long long n_pts, const long long *pair_off,
                      const long long *track_off, const int *track_img, const double *centres, const float *xyz,
                      unsigned long long *keys) {
  if (n_slots <= 0) return;
  hipLaunchKernelGGL(k_sfm_pairs, dim3(grid_of(n_slots)), dim3(kSfmBlock), 0, st, n_slots, n_pts, pair_off, track_off,
                     track_img, centres, xyz, keys);
}

void launch_sfm_segments(hipStream_t st, long long n_slots, const unsigned long long *keys, SfmPair *out,
                         unsigned long long capacity, unsigned long long *counter) {
  if (n_slots <= 0) return;
  hipLaunchKernelGGL(k_sfm_segments, dim3(grid_of(n_slots)), dim3(kSfmBlock), 0, st, n_slots, keys, out, capacity,
                     counter);
}

void launch_sfm_partners(hipStream_t st, int fill, long long n_pairs, const SfmPair *pairs, unsigned *cnt,
                         const long long *off, unsigned *part) {
  if (n_pairs <= 0) return;
  if (fill)
    hipLaunchKernelGGL(k_sfm_partners<1>, dim3(grid_of(n_pairs)), dim3(kSfmBlock), 0, st, n_pairs, pairs, cnt, off,
                       part);
  else
    hipLaunchKernelGGL(k_sfm_partners<0>, dim3(grid_of(n_pairs)), dim3(kSfmBlock), 0, st, n_pairs, pairs, cnt, off,
                       part);
}

void launch_sfm_scan(hipStream_t st, int n, const unsigned *cnt, long long *off) {
  hipLaunchKernelGGL(k_sfm_scan, dim3(1), dim3(kSfmScanBlock), 0, st, n, cnt, off);
}

void launch_sfm_select(hipStream_t st, int n_img, const long long *off, unsigned *part, double *score,
                       const SfmPair *pairs, const int *n_pts, int kind, float min_angle, long long num_images,
                       unsigned *nb, unsigned *nb_cnt) {
  if (n_img <= 0) return;
  hipLaunchKernelGGL(k_sfm_select, dim3((unsigned)n_img), dim3(64), 0, st, off, part, score, pairs, n_pts, kind,
                     min_angle, num_images, nb, nb_cnt);
}

void launch_sfm_compact(hipStream_t st, int n_img, const long long *off, const unsigned *nb, const unsigned *nb_cnt,
                        const long long *nb_off, int *dense) {
  if (n_img <= 0) return;
  hipLaunchKernelGGL(k_sfm_compact, dim3((unsigned)n_img), dim3(64), 0, st, off, nb, nb_cnt, nb_off, dense);
}

}  // namespace lt
