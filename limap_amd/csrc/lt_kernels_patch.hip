// lt_kernels_patch.hip -- device side of the line patch extraction (limap.features).
//   k_patch_gather<Tin, Tout, VEC>  all patches of one feature map in one launch.  Patches differ in their number of
//                    rows, so the host builds a table of (patch, first row, rows) blocks and a workgroup takes one entry:
//                    no lane searches for its patch.  A lane item is one texel's group of VEC consecutive channels; items
//                    are numbered channel group first, then x across the line, then y along it, which is the order of
//                    the output array (y, x, c): consecutive lanes store consecutive addresses, and a wave's loads of
//                    one neighbour are whole runs of the map's channels.
//                    VEC > 1 is the vector form: a lane owns 16 bytes of input channels (8 binary16, 4 float, 2 double),
//                    loads its four neighbours as four 16-byte words before it uses the first, and stores VEC outputs as
//                    16-byte words where they fill one (one 8- or 4-byte word otherwise).  VEC == 1 is the scalar form,
//                    one lane per (texel, channel) through the map's three strides: any channel count, any layout.
//                    The weights are recomputed per lane from lt_patch.h's expressions, so no bit depends on the mapping.
//                    Plain loads and stores only; nothing is atomic.
//   k_patch_copy16   the measurement's yardstick: 16 bytes per lane, nothing else.

#include "lt_patch.h"

namespace lt {

namespace {

__device__ __forceinline__ double pt_widen(unsigned short v) { return pt_half_bits_to_double(v); }
__device__ __forceinline__ double pt_widen(float v) { return (double)v; }
__device__ __forceinline__ double pt_widen(double v) { return v; }

__device__ __forceinline__ void pt_narrow(double v, unsigned short &o) { o = pt_double_to_half_bits(v); }
__device__ __forceinline__ void pt_narrow(double v, float &o) { o = pt_double_to_float(v); }
__device__ __forceinline__ void pt_narrow(double v, double &o) { o = v; }

template <class Tin, int VEC>
__device__ __forceinline__ void pt_load(const Tin *__restrict__ p, Tin (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = *p;
  } else {
    static_assert(VEC * sizeof(Tin) == 16, "a lane of the vector form owns 16 bytes of input");
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    __builtin_memcpy(v, &q, 16);
  }
}

// VEC outputs at an address that is a multiple of min(16, VEC * sizeof(Tout))
template <class Tout, int VEC>
__device__ __forceinline__ void pt_store(Tout *__restrict__ p, const Tout (&v)[VEC]) {
  constexpr int kBytes = VEC * (int)sizeof(Tout);
  if constexpr (kBytes % 16 == 0) {
    uint4 q[kBytes / 16];
    __builtin_memcpy(q, v, kBytes);
#pragma unroll
    for (int k = 0; k < kBytes / 16; ++k) reinterpret_cast<uint4 *>(p)[k] = q[k];
  } else if constexpr (kBytes == 8 && VEC > 1) {
    uint2 q;
    __builtin_memcpy(&q, v, 8);
    *reinterpret_cast<uint2 *>(p) = q;
  } else if constexpr (kBytes == 4 && VEC > 1) {
    unsigned q;
    __builtin_memcpy(&q, v, 4);
    *reinterpret_cast<unsigned *>(p) = q;
  } else {
    static_assert(VEC == 1, "store shape");
    p[0] = v[0];
  }
}

template <class Tin, class Tout, int VEC>
__global__ void __launch_bounds__(kPtBlock) k_patch_gather(const PtMap map, const int patch_w, const int n_blocks,
                                                           const PtBlock *__restrict__ blocks,
                                                           const PtPatch *__restrict__ patches,
                                                           Tout *__restrict__ out) {
  if ((int)blockIdx.x >= n_blocks) return;
  const PtBlock b = blocks[blockIdx.x];
  const PtPatch p = patches[b.patch];
  const int G = map.c / VEC;                 // channel groups of a texel
  const int per_row = patch_w * G;           // lane items of one patch row (the host keeps patch_w * c below 2^24)
  const int n_items = b.rows * per_row;      // (and rows * per_row below 2^31)
  const Tin *__restrict__ base = static_cast<const Tin *>(map.ptr);
  Tout *__restrict__ o = out + p.out_off + (long long)b.y0 * per_row * VEC;
  for (int e = (int)threadIdx.x; e < n_items; e += kPtBlock) {
    const int t = e / G, cg = e - t * G;
    const int yy = t / patch_w, x = t - yy * patch_w;
    double gx, gy;
    pt_global(p, x, b.y0 + yy, gx, gy);
    const PtTaps tp = pt_taps(gx, gy, map.h, map.w);
    const long long ch = (long long)cg * VEC * map.chan_stride;
    const Tin *r0 = base + (long long)tp.r0 * map.row_stride + ch;
    const Tin *r1 = base + (long long)tp.r1 * map.row_stride + ch;
    const long long c0 = (long long)tp.c0 * map.pix_stride, c1 = (long long)tp.c1 * map.pix_stride;
    Tin ll[VEC], lr[VEC], ul[VEC], ur[VEC];
    pt_load<Tin, VEC>(r0 + c0, ll);
    pt_load<Tin, VEC>(r0 + c1, lr);
    pt_load<Tin, VEC>(r1 + c0, ul);
    pt_load<Tin, VEC>(r1 + c1, ur);
    Tout res[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      pt_narrow(pt_blend(tp.dx, tp.dy, pt_widen(ll[k]), pt_widen(lr[k]), pt_widen(ul[k]), pt_widen(ur[k])), res[k]);
    pt_store<Tout, VEC>(o + (long long)e * VEC, res);
  }
}

__global__ void __launch_bounds__(kPtBlock) k_patch_copy16(long long n16, const uint4 *__restrict__ src,
                                                           uint4 *__restrict__ dst) {
  const long long i = (long long)blockIdx.x * kPtBlock + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

template <class Tin, class Tout>
void launch_io(hipStream_t st, const PtMap &map, int vec, int patch_w, int n_blocks, const PtBlock *blocks,
               const PtPatch *patches, void *out) {
  constexpr int kVec = 16 / (int)sizeof(Tin);
  if (vec)
    hipLaunchKernelGGL((k_patch_gather<Tin, Tout, kVec>), dim3((unsigned)n_blocks), dim3(kPtBlock), 0, st, map, patch_w,
                       n_blocks, blocks, patches, static_cast<Tout *>(out));
  else
    hipLaunchKernelGGL((k_patch_gather<Tin, Tout, 1>), dim3((unsigned)n_blocks), dim3(kPtBlock), 0, st, map, patch_w,
                       n_blocks, blocks, patches, static_cast<Tout *>(out));
}

template <class Tin>
void launch_in(hipStream_t st, const PtMap &map, int out_dtype, int vec, int patch_w, int n_blocks,
               const PtBlock *blocks, const PtPatch *patches, void *out) {
  if (out_dtype == kPtF16) launch_io<Tin, unsigned short>(st, map, vec, patch_w, n_blocks, blocks, patches, out);
  else if (out_dtype == kPtF32) launch_io<Tin, float>(st, map, vec, patch_w, n_blocks, blocks, patches, out);
  else if (out_dtype == kPtF64) launch_io<Tin, double>(st, map, vec, patch_w, n_blocks, blocks, patches, out);
}

}  // namespace

void launch_patch_gather(hipStream_t st, const PtMap &map, int out_dtype, int vec, int patch_w, int n_blocks,
                         const PtBlock *blocks, const PtPatch *patches, void *out) {
  if (n_blocks <= 0) return;
  if (map.dtype == kPtF16) launch_in<unsigned short>(st, map, out_dtype, vec, patch_w, n_blocks, blocks, patches, out);
  else if (map.dtype == kPtF32) launch_in<float>(st, map, out_dtype, vec, patch_w, n_blocks, blocks, patches, out);
  else if (map.dtype == kPtF64) launch_in<double>(st, map, out_dtype, vec, patch_w, n_blocks, blocks, patches, out);
}

void launch_patch_copy16(hipStream_t st, long long n16, const void *src, void *dst) {
  if (n16 <= 0) return;
  hipLaunchKernelGGL(k_patch_copy16, dim3((unsigned)((n16 + kPtBlock - 1) / kPtBlock)), dim3(kPtBlock), 0, st, n16,
                     static_cast<const uint4 *>(src), static_cast<uint4 *>(dst));
}

}  // namespace lt
