// est_host_asan.cpp -- the host twin of the minimal pose solvers (lt_fn_est_minimal_host of lt_est.cpp) under
// AddressSanitizer and UBSan, as a program of its own: lt_est.cpp is compiled into it with LT_HOST_ONLY and the
// sanitizers; nothing is loaded into Python and no device is touched.  `make -C limap_amd/csrc est_asan` builds and runs it.
// The cases: planted poses of every kind at 1, 63, 64, 65 and 257 samples with the planted pose looked for among the
// results; 1 against 4 threads; the degenerate samples (identical correspondences, collinear points, parallel lines,
// zero vectors, a half turn); the refusals; the hybrid loop (lt_fn_est_host) on planted queries of unequal size with one
// that VerifyData rejects, with the trace, at round sizes 1, 64 and 100, 1 against 3 threads, and its refusals.  Every
// array is exactly as long as the call may read or write.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

bool has(const char *what) { return host_asan::has(lt_fn_est_host_error, what); }

double uniform(unsigned &state) {  // [0, 1)
  state = state * 1664525u + 1013904223u;
  return (double)(state >> 8) / 16777216.0;
}

struct V3 { double v[3]; };
V3 unit(V3 a) {
  const double n = std::sqrt(a.v[0] * a.v[0] + a.v[1] * a.v[1] + a.v[2] * a.v[2]);
  return {{a.v[0] / n, a.v[1] / n, a.v[2] / n}};
}
V3 cross(V3 a, V3 b) {
  return {{a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]}};
}

struct Pose { double R[3][3], t[3]; };
Pose random_pose(unsigned &st, bool half_turn) {
  double q[4] = {half_turn ? 0.0 : uniform(st) - 0.5, uniform(st) - 0.5, uniform(st) - 0.5, uniform(st) - 0.5};
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  Pose p = {{{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
             {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
             {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}},
            {2 * uniform(st) - 1, 2 * uniform(st) - 1, 2 * uniform(st) - 1}};
  return p;
}
V3 cam_point(unsigned &st) {
  const double d = 2 + 4 * uniform(st);
  return {{(2 * uniform(st) - 1) * d, (2 * uniform(st) - 1) * d, d}};
}
V3 to_world(const Pose &p, V3 c) {  // R^T (c - t)
  V3 o;
  for (int i = 0; i < 3; ++i)
    o.v[i] = p.R[0][i] * (c.v[0] - p.t[0]) + p.R[1][i] * (c.v[1] - p.t[1]) + p.R[2][i] * (c.v[2] - p.t[2]);
  return o;
}

struct Batch {
  int kind = 0;
  std::vector<double> xs, Xs, ls, Cs, Vs;
  std::vector<Pose> truth;
  int64_t n() const { return (int64_t)truth.size(); }
};
void put(std::vector<double> &a, V3 v) { a.insert(a.end(), v.v, v.v + 3); }

Batch make(int kind, int n, unsigned seed, bool half_turn = false) {
  Batch b;
  b.kind = kind;
  unsigned st = seed;
  for (int i = 0; i < n; ++i) {
    const Pose p = random_pose(st, half_turn);
    for (int k = 0; k < 3 - kind; ++k) {
      const V3 c = cam_point(st);
      put(b.xs, unit(c));
      put(b.Xs, to_world(p, c));
    }
    for (int k = 0; k < kind; ++k) {
      const V3 a = cam_point(st), e = cam_point(st);
      const V3 A = to_world(p, a), B = to_world(p, e);
      const V3 V = unit({{B.v[0] - A.v[0], B.v[1] - A.v[1], B.v[2] - A.v[2]}});
      put(b.ls, unit(cross(unit(a), unit(e))));
      put(b.Cs, {{A.v[0] + 0.7 * V.v[0], A.v[1] + 0.7 * V.v[1], A.v[2] + 0.7 * V.v[2]}});
      put(b.Vs, V);
    }
    b.truth.push_back(p);
  }
  return b;
}

// exact-size outputs; the pointers of a kind without such data are null
int solve(const Batch &b, int threads, std::vector<double> &poses, std::vector<int32_t> &counts) {
  poses.assign(56 * (size_t)b.n(), -1.0);
  counts.assign((size_t)b.n(), -1);
  return lt_fn_est_minimal_host(b.kind, b.n(), b.xs.empty() ? nullptr : b.xs.data(), b.Xs.empty() ? nullptr : b.Xs.data(),
                                b.ls.empty() ? nullptr : b.ls.data(), b.Cs.empty() ? nullptr : b.Cs.data(),
                                b.Vs.empty() ? nullptr : b.Vs.data(), threads, poses.data(), counts.data());
}

int found(const Batch &b, const std::vector<double> &poses, const std::vector<int32_t> &counts) {
  int hits = 0;
  for (int64_t i = 0; i < b.n(); ++i) {
    bool hit = false;
    for (int s = 0; s < counts[(size_t)i]; ++s) {
      const double *q = &poses[(size_t)(56 * i + 7 * s)];
      const double w = q[0], x = q[1], y = q[2], z = q[3];
      const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                              {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                              {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
      double e = 0.0;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) e += std::fabs(R[r][c] - b.truth[(size_t)i].R[r][c]);
        e += std::fabs(q[4 + r] - b.truth[(size_t)i].t[r]);
      }
      hit = hit || e < 1e-6;
    }
    hits += hit;
  }
  return hits;
}

bool all_finite(const std::vector<double> &v) {
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

}  // namespace

int main() {
  std::vector<double> p1, p4;
  std::vector<int32_t> c1, c4;
  for (int kind = 0; kind < 4; ++kind)
    for (int n : {1, 63, 64, 65, 257}) {
      const Batch b = make(kind, n, 17u * (unsigned)n + (unsigned)kind);
      EXPECT(solve(b, 1, p1, c1) == LT_OK && solve(b, 4, p4, c4) == LT_OK);
      EXPECT(p1 == p4 && c1 == c4 && all_finite(p1));
      EXPECT(found(b, p1, c1) * 100 >= 95 * n);
      for (int32_t c : c1) EXPECT(c >= 0 && c <= LT_EST_MAX_SOLUTIONS);
    }
  // the degenerate samples
  for (int kind = 0; kind < 4; ++kind) {
    Batch b = make(kind, 4, 5u + (unsigned)kind, true);  // half turns: outside the chart
    EXPECT(solve(b, 2, p1, c1) == LT_OK && all_finite(p1));
    b = make(kind, 4, 9u + (unsigned)kind);
    if (kind < 2) {  // two identical points
      for (int c = 0; c < 3; ++c) { b.xs[3 + c] = b.xs[c]; b.Xs[3 + c] = b.Xs[c]; }
    }
    if (kind >= 2) {  // two identical lines; parallel directions in the next sample
      for (int c = 0; c < 3; ++c) { b.ls[3 + c] = b.ls[c]; b.Cs[3 + c] = b.Cs[c]; b.Vs[3 + c] = b.Vs[c]; }
      for (int k = 1; k < kind; ++k)
        for (int c = 0; c < 3; ++c) b.Vs[(size_t)(3 * kind + 3 * k + c)] = b.Vs[(size_t)(3 * kind + c)];
    }
    EXPECT(solve(b, 2, p1, c1) == LT_OK && all_finite(p1));
    b = make(kind, 2, 3u + (unsigned)kind);  // zero vectors
    if (kind < 3) for (int c = 0; c < 3; ++c) b.xs[c] = 0.0;
    if (kind > 0) for (int c = 0; c < 3; ++c) b.ls[c] = b.Vs[c] = 0.0;
    EXPECT(solve(b, 2, p1, c1) == LT_OK && all_finite(p1) && c1[0] == 0);
    if (kind == 0) {  // three collinear world points
      b = make(0, 1, 21u);
      for (int c = 0; c < 3; ++c) {
        b.Xs[6 + c] = 0.3 * b.Xs[c] + 0.7 * b.Xs[3 + c];
      }
      EXPECT(solve(b, 1, p1, c1) == LT_OK && all_finite(p1));
    }
  }
  // the refusals, and the empty batch
  {
    Batch b = make(1, 2, 1u);
    EXPECT(lt_fn_est_minimal_host(7, 2, b.xs.data(), b.Xs.data(), b.ls.data(), b.Cs.data(), b.Vs.data(), 1, nullptr, nullptr) == LT_ERR_ARGUMENT && has("unknown solver kind"));
    EXPECT(lt_fn_est_minimal_host(1, 2, b.xs.data(), b.Xs.data(), nullptr, b.Cs.data(), b.Vs.data(), 1, nullptr, nullptr) == LT_ERR_ARGUMENT && has("null"));
    EXPECT(lt_fn_est_minimal_host(1, -1, b.xs.data(), b.Xs.data(), b.ls.data(), b.Cs.data(), b.Vs.data(), 1, nullptr, nullptr) == LT_ERR_ARGUMENT && has("count"));
    b.Cs[4] = std::nan("");
    EXPECT(solve(b, 1, p1, c1) == LT_ERR_ARGUMENT && has("non-finite"));
    EXPECT(lt_fn_est_minimal_host(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr) == LT_OK);
    b = make(3, 3, 2u);
    EXPECT(lt_fn_est_minimal_host(3, 3, nullptr, nullptr, b.ls.data(), b.Cs.data(), b.Vs.data(), 0, nullptr, c1.data()) == LT_OK);
  }
  // the hybrid loop
  {
    const int n_pts[3] = {14, 1, 30}, n_seg[3] = {9, 1, 40};
    std::vector<double> k, q, t, p3, p2, l3, sg;
    std::vector<int64_t> po{0}, lo{0}, so{0};
    std::vector<int32_t> ids;
    unsigned st = 99u;
    for (int qi = 0; qi < 3; ++qi) {
      const Pose P = random_pose(st, false);
      const double kk[4] = {600, 590, 400, 300}, qq[4] = {1, 0, 0, 0}, tt[3] = {0, 0, 0};
      k.insert(k.end(), kk, kk + 4); q.insert(q.end(), qq, qq + 4); t.insert(t.end(), tt, tt + 3);
      auto pix = [&](V3 c, double *o) { o[0] = kk[0] * c.v[0] / c.v[2] + kk[2]; o[1] = kk[1] * c.v[1] / c.v[2] + kk[3]; };
      for (int i = 0; i < n_pts[qi]; ++i) {
        const V3 c = cam_point(st), w = to_world(P, c);
        double o[2];
        pix(i % 3 == 0 ? cam_point(st) : c, o);  // every third match is wrong
        p3.insert(p3.end(), w.v, w.v + 3); p2.insert(p2.end(), o, o + 2);
      }
      const int n_l3 = (n_seg[qi] + 1) / 2;  // two segments per 3D line
      std::vector<V3> ea, eb;
      for (int i = 0; i < n_l3; ++i) {
        V3 a = cam_point(st), b = cam_point(st);
        ea.push_back(a); eb.push_back(b);
        const V3 A = to_world(P, a), B = to_world(P, b);
        l3.insert(l3.end(), A.v, A.v + 3); l3.insert(l3.end(), B.v, B.v + 3);
      }
      for (int i = 0; i < n_seg[qi]; ++i) {
        double o[4];
        pix(i % 4 == 0 ? cam_point(st) : ea[(size_t)(i % n_l3)], o);
        pix(eb[(size_t)(i % n_l3)], o + 2);
        sg.insert(sg.end(), o, o + 4);
        ids.push_back(i % n_l3);
      }
      po.push_back((int64_t)p3.size() / 3); lo.push_back((int64_t)l3.size() / 6); so.push_back((int64_t)sg.size() / 4);
    }
    lt_est_config cfg;
    lt_est_config_default(&cfg);
    EXPECT(cfg.round_size == 64 && cfg.lo_starting_iterations == 50 && cfg.num_lsq_iterations == 4);
    cfg.squared_inlier_thresholds[0] = cfg.squared_inlier_thresholds[1] = 100.0;
    cfg.final_least_squares = 1;
    const int64_t cap = 40, N = po[3] + so[3];
    std::vector<double> ref_pose;
    for (int rs : {64, 1, 100})
      for (int threads : {1, 3}) {
        cfg.round_size = rs;
        std::vector<double> pose(21, -1.0), ds(9, -1.0), tr((size_t)(3 * cap * LT_EST_TRACE_DOUBLES), -1.0);
        std::vector<int32_t> is(36, -1), inl((size_t)N, -1);
        EXPECT(lt_fn_est_host(3, k.data(), q.data(), t.data(), po.data(), p3.data(), p2.data(), lo.data(), l3.data(), so.data(),
                              ids.data(), sg.data(), &cfg, cap, threads, pose.data(), ds.data(), is.data(), inl.data(), tr.data()) == LT_OK);
        EXPECT(all_finite(pose) && is[10] == 1 && is[12 + 10] == 0 && is[12] == 0 && is[24 + 10] == 1 && is[0] >= 100);
        EXPECT(pose[7] == 1.0 && pose[8] == 0.0 && is[5] >= 8 && is[24 + 5] >= 30);  // the rejected query keeps its pose
        if (threads == 1) ref_pose = pose;
        else EXPECT(pose == ref_pose);
      }
    EXPECT(lt_fn_est_host(3, k.data(), q.data(), t.data(), po.data(), p3.data(), p2.data(), lo.data(), l3.data(), so.data(), ids.data(),
                          sg.data(), &cfg, 0, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == LT_OK);
    cfg.round_size = 0;
    EXPECT(lt_fn_est_host(3, k.data(), q.data(), t.data(), po.data(), p3.data(), p2.data(), lo.data(), l3.data(), so.data(), ids.data(),
                          sg.data(), &cfg, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == LT_ERR_ARGUMENT && has("round_size"));
    cfg.round_size = 64;
    ids[0] = 1000;
    EXPECT(lt_fn_est_host(3, k.data(), q.data(), t.data(), po.data(), p3.data(), p2.data(), lo.data(), l3.data(), so.data(), ids.data(),
                          sg.data(), &cfg, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == LT_ERR_ARGUMENT && has("l3d_id"));
  }
  return finish("est_host_asan");
}
