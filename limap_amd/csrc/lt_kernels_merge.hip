// lt_kernels_merge.hip -- the pair tests of MergeToLineTracks (merging/merging.cc:347-511) on the GPU.
//
// One workgroup per (image, neighbour slot, tile of 256 rows); slot -1 is the self pass of the image (:389-414).
// Each thread owns one line of the image (a row) and walks the neighbour image's lines, whose unit directions and
// lengths are staged in LDS in chunks of kMergeChunk.  Per pair, in the reference's order:
//   parity rule of the cross pass (:431-435), zero-length neighbour line (:437-438), check_connection_3d (:441),
//   check_connection_2d of l1's projection into the neighbour view against the neighbour's segment (:444-447),
//   check_connection_2d of l2's projection into the own view against the own segment (:448-451);
//   self pass: check_connection_3d, then check_connection_2d of the two segments (:404-409).
// Before the exact 3D test a cosine guard rejects pairs whose |cos| lies below cos(th_angle (1 + 1e-6) + 1e-6 deg):
// the |cos| it reads is bit for bit the one angle_between computes (same unit directions, same dot), so it can never
// reject a pair the exact `acos(|cos|) * 180 / pi <= th_angle` accepts.  Accepted pairs are compacted per wave with a
// ballot and appended to the edge buffer with one atomic per wave; the counter runs on past `capacity` so that the host
// sees an overflow and runs again with a buffer of the counted size.  The host restores the reference's order.
#include "lt_devfn.h"

using namespace lt;

namespace {

constexpr int kMergeChunk = 1024;  // neighbour lines per LDS stage: 32 B each

template <bool kSelf>
__global__ __launch_bounds__(256) void k_merge_pairs(const MBlock *__restrict__ blks,
                                                     const long long *__restrict__ seg_off,
                                                     const MLine *__restrict__ lines, const Cam *__restrict__ cams,
                                                     LinkCfg2 l2, LinkCfg3 l3, double cos_guard, int parity_fast,
                                                     MEdge *__restrict__ edges, unsigned long long capacity,
                                                     unsigned long long *__restrict__ n_edges) {
  __shared__ double s_dl[kMergeChunk][4];  // neighbour lines: unit direction, length
  const MBlock b = blks[blockIdx.x];
  const long long base_i = seg_off[b.img], base_j = seg_off[b.nb];
  const int n_rows = (int)(seg_off[b.img + 1] - base_i);
  const int n_nb = (int)(seg_off[b.nb + 1] - base_j);
  const int i = b.row0 + (int)threadIdx.x;
  const int lane = lane_id();
  bool live = i < n_rows;
  MLine li;
  if (live) {
    li = lines[base_i + i];
    live = li.len != 0.0;
  }
  if (__syncthreads_or(live ? 1 : 0) == 0) return;
  const d3 di = live ? mk3(li.dir[0], li.dir[1], li.dir[2]) : mk3(0, 0, 0);
  // cross pass: key = image_id + line_id + ng_image_id + ng_line_id; skip if key is even and image_id < ng_image_id,
  // skip if key is odd and image_id > ng_image_id.  The ids compare as size_t (:434-435 compare int with size_t), the
  // key is the int the sum converts to.  parity_fast (all ids >= 0, every key below 2^31): with image_id !=
  // ng_image_id exactly one parity of ng_line_id remains, so a row walks every second neighbour line.
  const unsigned long long uimg = (unsigned long long)(long long)b.img_id;
  const unsigned long long unb = (unsigned long long)(long long)b.nb_id;
  const bool stride2 = !kSelf && parity_fast && b.img_id != b.nb_id;
  int jpar = 0;
  if (stride2) {
    const int want_odd = uimg < unb ? 1 : 0;  // image_id < ng_image_id keeps odd keys, image_id > ng_image_id even ones
    jpar = (int)(((unsigned)(b.img_id + i + b.nb_id) & 1u) ^ (unsigned)want_odd);
  }
  const Cam *cam_img = cams + b.img;
  const Cam *cam_nb = cams + b.nb;
  const double nodep[2] = {0.0, 0.0};  // depths: read by the scale-invariant gate only, which spatial merging disables
  for (int j0 = 0; j0 < n_nb; j0 += kMergeChunk) {
    const int j1 = min(n_nb, j0 + kMergeChunk);
    if (kSelf && j1 <= b.row0 + 1) continue;  // (uniform) every j of the chunk lies below every row of the tile
    __syncthreads();
    for (int k = (int)threadIdx.x; k < j1 - j0; k += (int)blockDim.x) {
      const MLine &q = lines[base_j + j0 + k];
      s_dl[k][0] = q.dir[0]; s_dl[k][1] = q.dir[1]; s_dl[k][2] = q.dir[2]; s_dl[k][3] = q.len;
    }
    __syncthreads();
    const int step = stride2 ? 2 : 1;
    const int n_iter = stride2 ? (j1 - j0 + 1) / 2 + 1 : j1 - j0;
    for (int it = 0; it < n_iter; ++it) {
      int j = stride2 ? j0 + ((j0 + jpar) & 1) + step * it : j0 + it;
      bool test = live && j < j1;
      if (test) {
        if (kSelf) {
          test = j > i;
        } else if (!stride2) {
          const unsigned long long sum = uimg + (unsigned long long)i + unb + (unsigned long long)j;
          const int key = (int)sum;
          if (key % 2 == 0 && uimg < unb) test = false;
          if (key % 2 == 1 && uimg > unb) test = false;
        }
      }
      if (test) {
        const int k = j - j0;
        test = s_dl[k][3] != 0.0;
        if (test && l3.use_angle) test = !(fabs(dot(di, mk3(s_dl[k][0], s_dl[k][1], s_dl[k][2]))) < cos_guard);
      }
      bool acc = false;
      if (test) {  // the reference's tests, in its order
        const MLine &lj = lines[base_j + j];
        const L3 a{mk3(li.s[0], li.s[1], li.s[2]), mk3(li.e[0], li.e[1], li.e[2])};
        const L3 c{mk3(lj.s[0], lj.s[1], lj.s[2]), mk3(lj.e[0], lj.e[1], lj.e[2])};
        acc = check3d(l3, a, c, li.unc, lj.unc, nodep);
        if (kSelf) {
          if (acc)
            acc = check2d(l2, L2{mk2(li.seg[0], li.seg[1]), mk2(li.seg[2], li.seg[3])},
                          L2{mk2(lj.seg[0], lj.seg[1]), mk2(lj.seg[2], lj.seg[3])});
        } else {
          if (acc)
            acc = check2d(l2, L2{cam_project(*cam_nb, a.s), cam_project(*cam_nb, a.e)},
                          L2{mk2(lj.seg[0], lj.seg[1]), mk2(lj.seg[2], lj.seg[3])});
          if (acc)
            acc = check2d(l2, L2{cam_project(*cam_img, c.s), cam_project(*cam_img, c.e)},
                          L2{mk2(li.seg[0], li.seg[1]), mk2(li.seg[2], li.seg[3])});
        }
      }
      const unsigned long long m = __ballot(acc);
      if (m) {
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(n_edges, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (acc) {
          const unsigned long long pos = base + (unsigned long long)__popcll(m & lanemask_lt());
          if (pos < capacity) edges[pos] = MEdge{b.img, i, b.slot, j};
        }
      }
    }
  }
}

}  // namespace

namespace lt {
void launch_merge_pairs(hipStream_t st, bool self, int n_blk, const MBlock *blks, const long long *seg_off,
                        const MLine *lines, const Cam *cams, const LinkCfg2 &l2, const LinkCfg3 &l3, double cos_guard,
                        int parity_fast, MEdge *edges, unsigned long long capacity, unsigned long long *n_edges) {
  if (n_blk <= 0) return;
  if (self)
    hipLaunchKernelGGL(k_merge_pairs<true>, dim3(n_blk), dim3(256), 0, st, blks, seg_off, lines, cams, l2, l3,
                       cos_guard, parity_fast, edges, capacity, n_edges);
  else
    hipLaunchKernelGGL(k_merge_pairs<false>, dim3(n_blk), dim3(256), 0, st, blks, seg_off, lines, cams, l2, l3,
                       cos_guard, parity_fast, edges, capacity, n_edges);
}
}  // namespace lt
