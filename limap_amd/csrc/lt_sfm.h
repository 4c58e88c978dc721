// lt_sfm.h -- records and the expressions shared by the host side (lt_sfm.cpp) and the device side (lt_kernels_sfm.hip)
// of the visual-neighbour computation (limap.pointsfm: SfmModel::GetMaxOverlapImages / GetMaxIoUImages /
// GetMaxDiceCoeffImages, pointsfm/sfm_model.cc over colmap::mvs::Model).  DESIGN §21 is the definition; both sides
// compile the same inline functions with -ffp-contract=off, so a key, a score or an order is the same bits on both.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lt {

constexpr int kSfmBlock = 256;          // lanes per workgroup of the per-slot / per-record kernels
constexpr int kSfmScanBlock = 1024;     // lanes of k_sfm_scan: one workgroup scans the per-image counts
constexpr int kSfmMaxImages = 65535;    // image indices take 16 bits of a key; 0xffff is the skipped slot's
constexpr unsigned kSfmDropped = 0x80000000u;  // k_sfm_select: set on the index of a partner the gate drops
constexpr unsigned long long kSfmSkipKey = ~0ull;  // a slot whose two track elements name the same image

// one unordered image pair i < j that shares a point: ij = i << 16 | j, the number of counted instances, the bits of
// the percentile angle (float32)
struct SfmPair {
  unsigned ij, shared, angle_bits, pad_;
};
static_assert(sizeof(SfmPair) == 16, "SfmPair layout");

#define LT_SFM_HD __host__ __device__ __forceinline__

LT_SFM_HD unsigned long long sfm_bits64(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
LT_SFM_HD double sfm_from_bits64(unsigned long long u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
LT_SFM_HD unsigned sfm_bits32(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
LT_SFM_HD float sfm_from_bits32(unsigned u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// acos on [-1, 1]: the rational approximation of fdlibm's e_acos.c (Sun Microsystems, freely distributable), written
// out so that the device and the host evaluate one sequence of IEEE operations (+, -, *, /, sqrt) instead of two
// libraries' acos.  Error below one ulp of the double result.
LT_SFM_HD double sfm_acos_r(double z) {
  const double p = z * (1.66666666666666657415e-01 +
                        z * (-3.25565818622400915405e-01 +
                             z * (2.01212532134862925881e-01 +
                                  z * (-4.00555345006794114027e-02 +
                                       z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
  const double q = 1.0 + z * (-2.40339491173441421878e+00 +
                              z * (2.02094576023350569471e+00 +
                                   z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
  return p / q;
}

LT_SFM_HD double sfm_acos(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
  const double pi = 3.14159265358979311600e+00;
  if (x >= 1.0) return 0.0;
  if (x <= -1.0) return pi + 2.0 * pio2_lo;
  const double ax = x < 0.0 ? -x : x;
  if (ax < 0.5) {
    if (ax < 0x1p-57) return pio2_hi + pio2_lo;
    return pio2_hi - (x - (pio2_lo - x * sfm_acos_r(x * x)));
  }
  if (x < 0.0) {
    const double z = (1.0 + x) * 0.5, s = sqrt(z);
    const double w = sfm_acos_r(z) * s - pio2_lo;
    return pi - 2.0 * (s + w);
  }
  const double z = (1.0 - x) * 0.5, s = sqrt(z);
  const double df = sfm_from_bits64(sfm_bits64(s) & 0xffffffff00000000ull);  // s with its low word cleared
  const double c = (z - df * df) / (s + df);
  const double w = sfm_acos_r(z) * s + c;
  return 2.0 * (df + w);
}

// CalculateTriangulationAngle of the projection centres ci, cj and the point x, all in double; the quotient is
// clamped to [-1, 1] (upstream hands acos a value outside it and gets NaN); narrowed to float32 as
// ComputeTriangulationAngles stores it.  The result is in [0, pi / 2]: its bits order like its value.
LT_SFM_HD float sfm_angle(const double *ci, const double *cj, double x, double y, double z) {
  const double bx = ci[0] - cj[0], by = ci[1] - cj[1], bz = ci[2] - cj[2];
  const double ux = x - ci[0], uy = y - ci[1], uz = z - ci[2];
  const double vx = x - cj[0], vy = y - cj[1], vz = z - cj[2];
  const double b2 = bx * bx + by * by + bz * bz;
  const double r1 = ux * ux + uy * uy + uz * uz;
  const double r2 = vx * vx + vy * vy + vz * vz;
  const double den = 2.0 * sqrt(r1 * r2);
  if (den == 0.0) return 0.0f;
  double q = (r1 + r2 - b2) / den;
  q = q < -1.0 ? -1.0 : (q > 1.0 ? 1.0 : q);
  const double pi = 3.14159265358979311600e+00;
  const double a = fabs(sfm_acos(q));
  const double b = pi - a;
  return (float)(a < b ? a : b);
}

// slot t of a track's lower triangle -> (a, b), a > b >= 0, t = a (a - 1) / 2 + b.  The square root is a first guess
// (exact in double for t < 2^50); the two loops make the decode exact whatever it returns.
LT_SFM_HD void sfm_tri_decode(long long t, long long *a_out, long long *b_out) {
  long long a = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
  if (a < 1) a = 1;
  while (a * (a - 1) / 2 > t) --a;
  while ((a + 1) * a / 2 <= t) ++a;
  *a_out = a;
  *b_out = t - a * (a - 1) / 2;
}

// the key of instance slot e: min(i, j) << 48 | max(i, j) << 32 | bits of the angle; kSfmSkipKey where i == j.
// pair_off[p] = slots of the points before p (pair_off[n_pts] = the number of slots, > e)
LT_SFM_HD unsigned long long sfm_slot_key(long long e, long long n_pts, const long long *pair_off,
                                          const long long *track_off, const int *track_img, const double *centres,
                                          const float *xyz) {
  long long lo = 0, hi = n_pts;  // pair_off[lo] <= e < pair_off[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (pair_off[mid] <= e) lo = mid; else hi = mid;
  }
  long long a, b;
  sfm_tri_decode(e - pair_off[lo], &a, &b);
  const int i = track_img[track_off[lo] + a], j = track_img[track_off[lo] + b];
  if (i == j) return kSfmSkipKey;
  const float ang = sfm_angle(centres + 3 * (long long)i, centres + 3 * (long long)j, (double)xyz[3 * lo],
                              (double)xyz[3 * lo + 1], (double)xyz[3 * lo + 2]);
  const unsigned long long mn = (unsigned long long)(i < j ? i : j), mx = (unsigned long long)(i < j ? j : i);
  return mn << 48 | mx << 32 | sfm_bits32(ang);
}

// element of the ascending angles of a pair the 75th percentile picks: round(0.75 (n - 1)), halves away from zero
LT_SFM_HD long long sfm_percentile_index(long long n) { return (3 * (n - 1) + 2) / 4; }

// kind: 0 overlap (GetMaxOverlappingImages), 1 IoU, 2 Dice coefficient.  shared >= 1 and IEEE division, so never NaN;
// a track that names its images more than once can make shared exceed n_i + n_j: the IoU is then negative, or +inf
LT_SFM_HD double sfm_score(int kind, unsigned shared, int n_i, int n_j) {
  const long long s = (long long)shared, both = (long long)n_i + (long long)n_j;
  if (kind == 1) return (double)s / (double)(both - s);
  if (kind == 2) return (double)(2 * s) / (double)both;
  return (double)s;
}

// the total order of the partners of one image: greater score first, then the smaller image index
LT_SFM_HD bool sfm_better(double s1, unsigned j1, double s2, unsigned j2) {
  return s1 > s2 || (s1 == s2 && j1 < j2);
}

void launch_sfm_pairs(hipStream_t st, long long n_slots, long long n_pts, const long long *pair_off,
                      const long long *track_off, const int *track_img, const double *centres, const float *xyz,
                      unsigned long long *keys);
// over the sorted keys: one record per run of equal upper 32 bits (the skipped slots' run excepted); *counter counts
// every record, those below `capacity` are stored
void launch_sfm_segments(hipStream_t st, long long n_slots, const unsigned long long *keys, SfmPair *out,
                         unsigned long long capacity, unsigned long long *counter);
// fill = 0: cnt[m] += records that name image m; fill = 1: part[off[m] + cursor[m]++] = record (any order)
void launch_sfm_partners(hipStream_t st, int fill, long long n_pairs, const SfmPair *pairs, unsigned *cnt,
                         const long long *off, unsigned *part);
// off[0 .. n] = exclusive sums of cnt[0 .. n)
void launch_sfm_scan(hipStream_t st, int n, const unsigned *cnt, long long *off);
// one wave per image: gate, score, rank.  part: in the records of the image's partners, out their image indices;
// score: scratch of the same extent (a dropped partner is marked on its index, not by its score); nb[off[m] + r] = partner of rank r < nb_cnt[m] = min(kept, num_images)
void launch_sfm_select(hipStream_t st, int n_img, const long long *off, unsigned *part, double *score,
                       const SfmPair *pairs, const int *n_pts, int kind, float min_angle, long long num_images,
                       unsigned *nb, unsigned *nb_cnt);
// dense[nb_off[m] ..) = nb[off[m] .. off[m] + nb_cnt[m])
void launch_sfm_compact(hipStream_t st, int n_img, const long long *off, const unsigned *nb, const unsigned *nb_cnt,
                        const long long *nb_off, int *dense);

}  // namespace lt
