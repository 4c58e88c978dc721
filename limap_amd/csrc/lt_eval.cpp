// lt_eval.cpp -- limap.evaluation on the GPU (evaluation/point_cloud_evaluator.cc, base_evaluator.cc,
// refline_evaluator.cc, mesh_evaluator.cc): the point index (lt_pcd_build), nearest-point distances of free points and
// of line samples (lt_pcd_nearest_dists, lt_pcd_line_samples), the point-to-segment minima of ComputeDistsforEachPoint
// (lt_lines_point_dists), the counters of RefLineEvaluator (lt_refline_counts), and the triangle index of
// MeshEvaluator with its point-to-mesh distances (lt_mesh_build, lt_mesh_nearest_dists, lt_mesh_line_samples).  The
// host validates, prepares the per-line constants (direction, length: the sqrt and divisions of Line3d, once per line)
// and launches in chunks; every distance is computed on the device (lt_kernels_eval.hip).  DESIGN §14, §15.

#include "lt_host.h"
#include "lt_eval.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

struct lt_pcd {
  static constexpr const char *noun = "index";  // of the messages about the handle
  int device = 0;
  long long n = 0;
  DevBuf x, y, z, box, perm;
  EvalTree tree{};
};

struct lt_mesh {
  static constexpr const char *noun = "mesh";
  int device = 0;
  long long n = 0;  // faces
  DevBuf faces, box, eta, perm;
  MeshTree tree{};
};

namespace {

constexpr long long kDefaultChunk = 1ll << 22;

long long chunk_of(int64_t chunk) { return chunk > 0 ? (long long)chunk : kDefaultChunk; }

// Line3d's direction() (Eigen normalized(): unchanged unless the squared norm is > 0) and length() ((start - end).norm())
std::vector<EvalLine> prep_lines(const double *l6, long long n, int rint_n) {
  std::vector<EvalLine> out((size_t)std::max<long long>(n, 1));
  for (long long k = 0; k < n; ++k) {
    const double *a = l6 + 6 * k;
    EvalLine &L = out[(size_t)k];
    double v[3], w[3];
    for (int c = 0; c < 3; ++c) {
      L.s[c] = a[c];
      L.e[c] = a[3 + c];
      v[c] = a[3 + c] - a[c];
      w[c] = a[c] - a[3 + c];
    }
    const double z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (z > 0.0) {
      const double nv = std::sqrt(z);
      for (int c = 0; c < 3; ++c) L.d[c] = v[c] / nv;
    } else {
      for (int c = 0; c < 3; ++c) L.d[c] = v[c];
    }
    L.len = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    L.rint = rint_n > 0 ? L.len / (double)(rint_n - 1) : 0.0;  // ComputeRecallLength: length() / (num_samples - 1)
    L.pad_ = 0.0;
  }
  return out;
}

template <class Handle>
int check_handle(lt_ctx *ctx, const char *who, const Handle *h) {
  if (!h) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": null " + Handle::noun);
  if (h->device != ctx->device)
    return fail(ctx, LT_ERR_ARGUMENT,
                std::string(who) + ": the " + Handle::noun + " lives on another device than the context");
  return LT_OK;
}

// LT_TEST_MESH_BRUTE=1: every face for every query (k_mesh_brute), the yardstick of the hierarchy walk
int mesh_brute() {
  const char *e = test_switch("LT_TEST_MESH_BRUTE");
  return e && e[0] == '1';
}

struct Timer {  // HIP events around the kernels of one call
  Events<2> ev;
  double t0 = now_ms();
  int launches = 0;
  int start(lt_ctx *ctx) {
    if (int rc = ev.create(ctx)) return rc;
    return ev.record(ctx, 0);
  }
  int finish(lt_ctx *ctx, double levels) {
    if (int rc = ev.record(ctx, 1)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    ctx->evl.timers[0] = ev.ms(0, 1);
    ctx->evl.timers[1] = now_ms() - t0;
    ctx->evl.timers[2] = launches;
    ctx->evl.timers[3] = levels;
    return LT_OK;
  }
};

// the nearest-distance launch of an index: (stream, queries, their number, distances out)
auto pcd_launch(const lt_pcd *pcd) {
  return [pcd](hipStream_t st, const EvalQuery &Q, long long nq, double *dist) {
    launch_eval_nearest(st, pcd->tree, Q, nq, dist);
  };
}

auto mesh_launch(const lt_mesh *mesh) {
  const int brute = mesh_brute();
  return [mesh, brute](hipStream_t st, const EvalQuery &Q, long long nq, double *dist) {
    launch_mesh_nearest(st, mesh->tree, Q, nq, brute, dist);
  };
}

// the Morton order of n device points: bounding box -> 21-bit quantisation per axis -> 63-bit Morton keys -> rocprim
// radix sort.  Scratch, carved at 256 bytes: six ordered keys of the box, Morton keys in and out, indices in, the sort's.
struct MortonOrder {
  long long n;
  size_t kb, ib, tmp;
  char *scr = nullptr;
  explicit MortonOrder(long long n_)
      : n(n_), kb(((size_t)n_ * 8 + 255) & ~(size_t)255), ib(((size_t)n_ * 4 + 255) & ~(size_t)255),
        tmp(eval_sort_temp_bytes(n_)) {}
  size_t bytes() const { return 256 + 2 * kb + ib + std::max<size_t>(tmp, 16); }
  // takes the scratch and uploads the box's initial keys: the last of a build's uploads, before its first kernel
  hipError_t prime(hipStream_t st, char *scratch) {
    static const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0, 0, 0};
    scr = scratch;
    return hipMemcpyAsync(scr, init, 48, hipMemcpyHostToDevice, st);
  }
  // the order into perm.  Synchronises the stream once (the box comes to the host); the sort is left in flight.
  int run(lt_ctx *ctx, const char *who, const void *xyz, int dtype, unsigned *perm, int *launches) const {
    hipStream_t st = ctx->stream;
    unsigned long long *box6 = reinterpret_cast<unsigned long long *>(scr);
    unsigned long long *k_in = reinterpret_cast<unsigned long long *>(scr + 256);
    unsigned long long *k_out = reinterpret_cast<unsigned long long *>(scr + 256 + kb);
    unsigned *i_in = reinterpret_cast<unsigned *>(scr + 256 + 2 * kb);
    launch_eval_bbox(st, xyz, dtype, n, box6);
    unsigned long long got[6];
    if (hipMemcpyAsync(got, box6, 48, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return fail(ctx, LT_ERR_HIP, std::string(who) + ": bounding box failed");
    double lo[3], scale[3];
    for (int k = 0; k < 3; ++k) {
      auto dec = [](unsigned long long u) {
        u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
        double v;
        std::memcpy(&v, &u, 8);
        return v;
      };
      lo[k] = dec(got[k]);
      const double ext = dec(got[3 + k]) - lo[k];
      scale[k] = (ext > 0.0 && std::isfinite(ext)) ? 2097151.0 / ext : 0.0;
    }
    launch_eval_morton(st, xyz, dtype, n, lo, scale, k_in, i_in);
    if (launch_eval_sort(st, scr + 256 + 2 * kb + ib, tmp, n, k_in, k_out, i_in, perm) != 0)
      return fail(ctx, LT_ERR_HIP, "rocprim radix sort failed");
    *launches += 3;
    return LT_OK;
  }
};

// nearest distances of free points, in chunks
template <class Launch>
int nearest_dists(lt_ctx *ctx, const char *who, const double *query, int64_t n, int64_t chunk, double *dist,
                  Launch launch) {
  if (n < 0 || (n > 0 && (!query || !dist))) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": bad arguments");
  if (int rc = check_finite(ctx, who, query, 3 * n, "query coordinate")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  const long long C = chunk_of(chunk);
  ENSURE(ctx, ctx->evl.d_in, 24 * (size_t)std::min<long long>(std::max<long long>(n, 1), C));
  ENSURE(ctx, ctx->evl.d_out, 8 * (size_t)std::min<long long>(std::max<long long>(n, 1), C));
  for (long long q0 = 0; q0 < n; q0 += C) {
    const long long m = std::min<long long>(C, n - q0);
    HIPCHK(ctx, hipMemcpyAsync(ctx->evl.d_in.p, query + 3 * q0, 24 * (size_t)m, hipMemcpyHostToDevice, st));
    EvalQuery Q{};
    const double *d = ctx->evl.d_in.as<double>();
    Q.x = d; Q.y = d + 1; Q.z = d + 2; Q.stride = 3; Q.mode = EV_Q_POINTS; Q.n = 1;
    launch(st, Q, m, ctx->evl.d_out.as<double>());
    ++tm.launches;
    HIPCHK(ctx, hipMemcpyAsync(dist + q0, ctx->evl.d_out.p, 8 * (size_t)m, hipMemcpyDeviceToHost, st));
  }
  return tm.finish(ctx, 0);
}

// nearest distances of the samples of lines, whole lines per launch, with optional per-threshold counts
template <class Launch>
int line_samples(lt_ctx *ctx, const char *who, const double *lines, int64_t n_lines, int mode, int n_samples,
                 const double *thresholds, int n_th, int64_t chunk, double *dists, int32_t *counts, Launch launch) {
  const std::string w(who);
  if (mode != LT_SAMPLE_CENTER && mode != LT_SAMPLE_ENDS) return fail(ctx, LT_ERR_ARGUMENT, w + ": bad mode");
  if (n_samples < (mode == LT_SAMPLE_ENDS ? 2 : 1))
    return fail(ctx, LT_ERR_ARGUMENT, w + ": n_samples must be >= 1 (>= 2 for end-point sampling)");
  if (n_th < 0 || n_th > kEvalMaxTh || (n_th > 0 && !thresholds))
    return fail(ctx, LT_ERR_ARGUMENT, w + ": between 0 and 64 thresholds");
  if (n_lines < 0 || (n_lines > 0 && !lines)) return fail(ctx, LT_ERR_ARGUMENT, w + ": bad lines");
  if (counts && n_th == 0) counts = nullptr;
  if (int rc = check_finite(ctx, who, lines, 6 * n_lines, "line coordinate")) return rc;
  if (n_lines == 0 || (!dists && !counts)) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  const auto L = prep_lines(lines, n_lines, 0);
  if (int rc = upload_vec(ctx, ctx->evl.d_lines, L)) return rc;
  ENSURE(ctx, ctx->evl.d_th, 8 * (size_t)std::max(n_th, 1));
  if (n_th) HIPCHK(ctx, hipMemcpyAsync(ctx->evl.d_th.p, thresholds, 8 * (size_t)n_th, hipMemcpyHostToDevice, st));
  const long long per = std::max<long long>(1, chunk_of(chunk) / n_samples);  // whole lines per launch
  const long long lc = std::min<long long>(per, n_lines);
  ENSURE(ctx, ctx->evl.d_out, 8 * (size_t)(lc * n_samples));
  if (counts) ENSURE(ctx, ctx->evl.d_cnt, 4 * (size_t)(n_lines * n_th));
  EvalQuery Q{};
  Q.mode = mode == LT_SAMPLE_CENTER ? EV_Q_CENTER : EV_Q_ENDS;
  Q.n = n_samples;
  Q.interval = mode == LT_SAMPLE_CENTER ? 1.0 / n_samples : 1.0 / (n_samples - 1);
  for (long long l0 = 0; l0 < n_lines; l0 += per) {
    const long long m = std::min<long long>(per, n_lines - l0);
    Q.lines = ctx->evl.d_lines.as<EvalLine>() + l0;
    launch(st, Q, m * n_samples, ctx->evl.d_out.as<double>());
    ++tm.launches;
    if (counts) {
      launch_eval_count(st, ctx->evl.d_out.as<double>(), m, n_samples, ctx->evl.d_th.as<double>(), n_th, 1,
                        ctx->evl.d_cnt.as<int>() + l0 * n_th);
      ++tm.launches;
    }
    if (dists)
      HIPCHK(ctx, hipMemcpyAsync(dists + l0 * n_samples, ctx->evl.d_out.p, 8 * (size_t)(m * n_samples),
                                 hipMemcpyDeviceToHost, st));
  }
  if (counts)
    HIPCHK(ctx, hipMemcpyAsync(counts, ctx->evl.d_cnt.p, 4 * (size_t)(n_lines * n_th), hipMemcpyDeviceToHost, st));
  return tm.finish(ctx, 0);
}

}  // namespace

extern "C" {

int lt_pcd_build(lt_ctx *ctx, const void *xyz, int64_t n, int dtype, int on_device, const uint32_t *perm,
                 lt_pcd **out) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  *out = nullptr;
  if (n <= 0) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: empty point cloud");
  if (n >= (1ll << 32)) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: more than 2^32 - 1 points");
  if (!xyz) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: null points");
  if (dtype != 0 && dtype != 1) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: dtype must be 0 (float32) or 1 (float64)");
  if (!on_device) {
    for (long long k = 0; k < 3 * n; ++k) {
      const double v = dtype ? static_cast<const double *>(xyz)[k] : (double)static_cast<const float *>(xyz)[k];
      if (!std::isfinite(v)) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: non-finite point coordinate");
    }
  }
  if (perm) {  // a saved order: any permutation gives exact answers, anything else would read out of bounds
    std::vector<unsigned char> seen((size_t)n, 0);
    for (long long k = 0; k < n; ++k) {
      if ((long long)perm[k] >= n || seen[perm[k]])
        return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_build: the saved order is not a permutation of the points");
      seen[perm[k]] = 1;
    }
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  lt_pcd *p = new lt_pcd();
  p->device = ctx->device;
  p->n = n;
  auto bail = [&](int rc) {
    (void)hipStreamSynchronize(st);
    delete p;
    return rc;
  };
  const size_t in_bytes = (size_t)n * 3 * (dtype ? 8 : 4);
  const void *src = xyz;
  if (!on_device) {
    if (!ctx->evl.d_in.ensure(in_bytes)) return bail(fail(ctx, LT_ERR_HIP, "hipMalloc failed for the point upload"));
    if (hipMemcpyAsync(ctx->evl.d_in.p, xyz, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
      return bail(fail(ctx, LT_ERR_HIP, "lt_pcd_build: upload failed"));
    src = ctx->evl.d_in.p;
  }
  EvalTree &T = p->tree;
  T.L = eval_levels(n, kEvalBucket);
  if (!p->x.ensure(8 * (size_t)n) || !p->y.ensure(8 * (size_t)n) || !p->z.ensure(8 * (size_t)n) ||
      !p->box.ensure(48 * (size_t)T.L.total) || !p->perm.ensure(4 * (size_t)n))
    return bail(fail(ctx, LT_ERR_HIP, "hipMalloc failed for the point index"));
  if (perm) {
    if (hipMemcpyAsync(p->perm.p, perm, 4 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess)
      return bail(fail(ctx, LT_ERR_HIP, "lt_pcd_build: upload of the order failed"));
  } else {
    DevBuf keys;
    MortonOrder order(n);
    if (!keys.ensure(order.bytes()))
      return bail(fail(ctx, LT_ERR_HIP, "hipMalloc failed for the sort of the point index"));
    if (order.prime(st, keys.as<char>()) != hipSuccess)
      return bail(fail(ctx, LT_ERR_HIP, "lt_pcd_build: memcpy failed"));
    if (int rc = order.run(ctx, "lt_pcd_build", src, dtype, p->perm.as<unsigned>(), &tm.launches)) return bail(rc);
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(ctx, LT_ERR_HIP, "lt_pcd_build: sort failed"));
  }
  T.x = p->x.as<double>();
  T.y = p->y.as<double>();
  T.z = p->z.as<double>();
  T.box = p->box.as<double>();
  launch_eval_gather(st, src, dtype, n, p->perm.as<unsigned>(), p->x.as<double>(), p->y.as<double>(),
                     p->z.as<double>());
  launch_eval_boxes(st, T, p->box.as<double>());
  tm.launches += 2 + T.L.top;
  if (int rc = tm.finish(ctx, T.L.top + 1)) return bail(rc);
  *out = p;
  return LT_OK;
}

void lt_pcd_free(lt_pcd *pcd) {
  if (!pcd) return;
  (void)hipSetDevice(pcd->device);
  (void)hipDeviceSynchronize();  // no work of any stream may still read the index
  delete pcd;
}

int lt_pcd_get_perm(lt_ctx *ctx, const lt_pcd *pcd, uint32_t *perm) {
  if (int rc = check_handle(ctx, "lt_pcd_get_perm", pcd)) return rc;
  if (!perm) return fail(ctx, LT_ERR_ARGUMENT, "lt_pcd_get_perm: null output");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(perm, pcd->perm.p, 4 * (size_t)pcd->n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return LT_OK;
}

int lt_pcd_nearest_dists(lt_ctx *ctx, const lt_pcd *pcd, const double *query, int64_t n, int64_t chunk,
                         double *dist) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_pcd_nearest_dists";
  if (int rc = check_handle(ctx, who, pcd)) return rc;
  return nearest_dists(ctx, who, query, n, chunk, dist, pcd_launch(pcd));
}

int lt_pcd_line_samples(lt_ctx *ctx, const lt_pcd *pcd, const double *lines, int64_t n_lines, int mode,
                        int n_samples, const double *thresholds, int n_th, int64_t chunk, double *dists,
                        int32_t *counts) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_pcd_line_samples";
  if (int rc = check_handle(ctx, who, pcd)) return rc;
  return line_samples(ctx, who, lines, n_lines, mode, n_samples, thresholds, n_th, chunk, dists, counts,
                      pcd_launch(pcd));
}

int lt_lines_point_dists(lt_ctx *ctx, const lt_pcd *pcd, const double *lines, int64_t n_lines, int64_t chunk,
                         double *dist) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_lines_point_dists";
  if (int rc = check_handle(ctx, who, pcd)) return rc;
  if (!dist || n_lines < 0 || (n_lines > 0 && !lines)) return fail(ctx, LT_ERR_ARGUMENT, "lt_lines_point_dists: bad arguments");
  if (int rc = check_finite(ctx, who, lines, 6 * n_lines, "line coordinate")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  const auto L = prep_lines(lines, n_lines, 0);
  if (int rc = upload_vec(ctx, ctx->evl.d_lines, L)) return rc;
  const long long N = pcd->n, C = chunk_of(chunk);
  ENSURE(ctx, ctx->evl.d_out, 8 * (size_t)N);
  for (long long p0 = 0; p0 < N; p0 += C) {  // the cloud in Morton order, written back in the input order
    const long long m = std::min<long long>(C, N - p0);
    EvalQuery Q{};
    Q.x = pcd->x.as<double>() + p0; Q.y = pcd->y.as<double>() + p0; Q.z = pcd->z.as<double>() + p0;
    Q.stride = 1; Q.mode = EV_Q_POINTS; Q.n = 1;
    launch_eval_lines_min(st, 0, Q, m, ctx->evl.d_lines.as<EvalLine>(), n_lines, ctx->evl.d_out.as<double>(),
                          pcd->perm.as<unsigned>() + p0);
    ++tm.launches;
  }
  HIPCHK(ctx, hipMemcpyAsync(dist, ctx->evl.d_out.p, 8 * (size_t)N, hipMemcpyDeviceToHost, st));
  return tm.finish(ctx, 0);
}

int lt_refline_counts(lt_ctx *ctx, const double *query_lines, int64_t n_query, const double *lines, int64_t n_lines,
                      int n_samples, const double *thresholds, int n_th, int64_t chunk, int32_t *counts) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_refline_counts";
  if (n_samples < 1) return fail(ctx, LT_ERR_ARGUMENT, "lt_refline_counts: n_samples must be >= 1");
  if (n_th < 0 || n_th > kEvalMaxTh || (n_th > 0 && !thresholds))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refline_counts: between 0 and 64 thresholds");
  if (n_query < 0 || n_lines < 0 || (n_query > 0 && !query_lines) || (n_lines > 0 && !lines) ||
      (n_query > 0 && n_th > 0 && !counts))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refline_counts: bad arguments");
  if (int rc = check_finite(ctx, who, query_lines, 6 * n_query, "line coordinate")) return rc;
  if (int rc = check_finite(ctx, who, lines, 6 * n_lines, "line coordinate")) return rc;
  if (n_query == 0 || n_th == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  const auto QL = prep_lines(query_lines, n_query, n_samples);
  const auto L = prep_lines(lines, n_lines, 0);
  if (int rc = upload_vec(ctx, ctx->evl.d_in, QL)) return rc;
  if (int rc = upload_vec(ctx, ctx->evl.d_lines, L)) return rc;
  ENSURE(ctx, ctx->evl.d_th, 8 * (size_t)n_th);
  HIPCHK(ctx, hipMemcpyAsync(ctx->evl.d_th.p, thresholds, 8 * (size_t)n_th, hipMemcpyHostToDevice, st));
  const long long per = std::max<long long>(1, chunk_of(chunk) / n_samples);
  ENSURE(ctx, ctx->evl.d_out, 8 * (size_t)(std::min<long long>(per, n_query) * n_samples));
  ENSURE(ctx, ctx->evl.d_cnt, 4 * (size_t)(n_query * n_th));
  EvalQuery Q{};
  Q.mode = EV_Q_REFLINE;
  Q.n = n_samples;
  for (long long r0 = 0; r0 < n_query; r0 += per) {
    const long long m = std::min<long long>(per, n_query - r0);
    Q.lines = ctx->evl.d_in.as<EvalLine>() + r0;
    launch_eval_lines_min(st, 1, Q, m * n_samples, ctx->evl.d_lines.as<EvalLine>(), n_lines,
                          ctx->evl.d_out.as<double>(), nullptr);
    launch_eval_count(st, ctx->evl.d_out.as<double>(), m, n_samples, ctx->evl.d_th.as<double>(), n_th, 0,
                      ctx->evl.d_cnt.as<int>() + r0 * n_th);
    tm.launches += 2;
  }
  HIPCHK(ctx, hipMemcpyAsync(counts, ctx->evl.d_cnt.p, 4 * (size_t)(n_query * n_th), hipMemcpyDeviceToHost, st));
  return tm.finish(ctx, 0);
}

int lt_mesh_build(lt_ctx *ctx, const void *V, int64_t nv, int dtype, int on_device, const int64_t *F, int64_t nf,
                  double scale, lt_mesh **out) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  *out = nullptr;
  const char *who = "lt_mesh_build";
  if (nf <= 0) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: a mesh without faces");
  if (nf >= (1ll << 32)) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: more than 2^32 - 1 faces");
  if (nv <= 0 || !V || !F) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: null or empty vertices or faces");
  if (dtype != 0 && dtype != 1) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: dtype must be 0 (float32) or 1 (float64)");
  if (!std::isfinite(scale)) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: non-finite scale");
  for (long long k = 0; k < 3 * nf; ++k)
    if (F[k] < 0 || F[k] >= nv) return fail(ctx, LT_ERR_ARGUMENT, "lt_mesh_build: face index out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the vertices as the reference scales them (V_ *= mpau): one multiplication per coordinate, here on the host
  const size_t in_bytes = (size_t)nv * 3 * (dtype ? 8 : 4);
  std::vector<unsigned char> staged;
  const void *src = V;
  if (on_device) {
    staged.resize(in_bytes);
    HIPCHK(ctx, hipMemcpy(staged.data(), V, in_bytes, hipMemcpyDeviceToHost));
    src = staged.data();
  }
  std::vector<double> Vs((size_t)nv * 3);
  for (long long k = 0; k < 3 * nv; ++k) {
    const double v = dtype ? static_cast<const double *>(src)[k] : (double)static_cast<const float *>(src)[k];
    Vs[(size_t)k] = v * scale;
    if (!std::isfinite(Vs[(size_t)k])) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": non-finite vertex coordinate");
  }
  int bucket = kMeshBucket;
  if (const char *e = test_switch("LT_TEST_MESH_BUCKET")) {  // bucket sizes for the measurement
    bucket = atoi(e);
    if (bucket < 1 || bucket > kMeshMaxBucket) return fail(ctx, LT_ERR_ARGUMENT, "LT_TEST_MESH_BUCKET: 1 .. 64");
  }
  Timer tm;
  if (int rc = tm.start(ctx)) return rc;
  lt_mesh *m = new lt_mesh();
  m->device = ctx->device;
  m->n = nf;
  auto bail = [&](int rc) {
    (void)hipStreamSynchronize(st);
    delete m;
    return rc;
  };
  MeshTree &T = m->tree;
  T.L = eval_levels(nf, bucket);
  T.bucket = bucket;
  // scratch: vertices, faces and centroids, then the order's
  MortonOrder order(nf);
  const size_t vb = ((size_t)nv * 24 + 255) & ~(size_t)255, fb = ((size_t)nf * 24 + 255) & ~(size_t)255;
  DevBuf scr;
  if (!scr.ensure(vb + 2 * fb + order.bytes()) || !m->faces.ensure(72 * (size_t)nf) ||
      !m->box.ensure(48 * (size_t)T.L.total) || !m->eta.ensure(8 * (size_t)T.L.total) ||
      !m->perm.ensure(4 * (size_t)nf))
    return bail(fail(ctx, LT_ERR_HIP, "hipMalloc failed for the mesh index"));
  char *sp = scr.as<char>();
  double *dV = reinterpret_cast<double *>(sp);
  long long *dF = reinterpret_cast<long long *>(sp + vb);
  double *cen = reinterpret_cast<double *>(sp + vb + fb);
  if (hipMemcpyAsync(dV, Vs.data(), 24 * (size_t)nv, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(dF, F, 24 * (size_t)nf, hipMemcpyHostToDevice, st) != hipSuccess ||
      order.prime(st, sp + vb + 2 * fb) != hipSuccess)
    return bail(fail(ctx, LT_ERR_HIP, "lt_mesh_build: upload failed"));
  // the order: the point index's, over the face centroids
  launch_mesh_centroids(st, dV, dF, nf, cen);
  if (int rc = order.run(ctx, who, cen, 1, m->perm.as<unsigned>(), &tm.launches)) return bail(rc);
  double *fa[9];
  for (int k = 0; k < 9; ++k) {
    fa[k] = m->faces.as<double>() + (size_t)k * nf;
    T.v[k] = fa[k];
  }
  T.box = m->box.as<double>();
  T.eta = m->eta.as<double>();
  launch_mesh_gather(st, dV, dF, nf, m->perm.as<unsigned>(), fa);
  launch_mesh_boxes(st, T, m->box.as<double>(), m->eta.as<double>());
  tm.launches += 3 + 2 * T.L.top;
  if (int rc = tm.finish(ctx, T.L.top + 1)) return bail(rc);  // (the scratch returns to the cache after the sync)
  *out = m;
  return LT_OK;
}

void lt_mesh_free(lt_mesh *mesh) {
  if (!mesh) return;
  (void)hipSetDevice(mesh->device);
  (void)hipDeviceSynchronize();
  delete mesh;
}

int lt_mesh_nearest_dists(lt_ctx *ctx, const lt_mesh *mesh, const double *query, int64_t n, int64_t chunk,
                          double *dist) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_mesh_nearest_dists";
  if (int rc = check_handle(ctx, who, mesh)) return rc;
  return nearest_dists(ctx, who, query, n, chunk, dist, mesh_launch(mesh));
}

int lt_mesh_line_samples(lt_ctx *ctx, const lt_mesh *mesh, const double *lines, int64_t n_lines, int mode,
                         int n_samples, const double *thresholds, int n_th, int64_t chunk, double *dists,
                         int32_t *counts) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_mesh_line_samples";
  if (int rc = check_handle(ctx, who, mesh)) return rc;
  return line_samples(ctx, who, lines, n_lines, mode, n_samples, thresholds, n_th, chunk, dists, counts,
                      mesh_launch(mesh));
}

int lt_eval_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->evl.timers[k];
  return LT_OK;
}

}  // extern "C"
