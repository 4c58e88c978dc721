// est_host_asan.cpp -- the host twin of the minimal pose solvers (lt_fn_est_minimal_host of lt_est.cpp) under
// AddressSanitizer and UBSan, as a program of its own: lt_est.cpp is compiled into it with LT_HOST_ONLY and the
// sanitizers; nothing is loaded into Python and no device is touched.  `make -C limap_amd/csrc est_asan` builds and runs it.
// The cases: planted poses of every kind at 1, 63, 64, 65 and 257 samples with the planted pose looked for among the
// results; 1 against 4 threads; the degenerate samples (identical correspondences, collinear points, parallel lines,
// zero vectors, a half turn); the refusals; the hybrid loop (lt_fn_est_host) on planted queries of unequal size with one
// that VerifyData rejects, with the trace, at round sizes 1, 64 and 100, 1 against 3 threads, a points-only, a lines-only
// and a three-point query (in one batch and alone), E3DLineLineDist2 with the Cauchy loss, and its refusals.  Every
// array is exactly as long as the call may read or write; a call without data of a kind passes null for it.
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

// planted queries of the hybrid loop in CSR form: every third point match and every fourth segment's start are wrong,
// two segments per 3D line; every array is exactly as long as its offsets say
struct Queries {
  std::vector<double> k, q, t, p3, p2, l3, sg;
  std::vector<int64_t> po{0}, lo{0}, so{0};
  std::vector<int32_t> ids;
  int64_t n() const { return (int64_t)po.size() - 1; }
  int64_t N() const { return po.back() + so.back(); }
};
Queries make_queries(const std::vector<int> &n_pts, const std::vector<int> &n_seg, unsigned seed) {
  Queries Q;
  unsigned st = seed;
  for (size_t qi = 0; qi < n_pts.size(); ++qi) {
    const Pose P = random_pose(st, false);
    const double kk[4] = {600, 590, 400, 300}, qq[4] = {1, 0, 0, 0}, tt[3] = {0, 0, 0};
    Q.k.insert(Q.k.end(), kk, kk + 4); Q.q.insert(Q.q.end(), qq, qq + 4); Q.t.insert(Q.t.end(), tt, tt + 3);
    auto pix = [&](V3 c, double *o) { o[0] = kk[0] * c.v[0] / c.v[2] + kk[2]; o[1] = kk[1] * c.v[1] / c.v[2] + kk[3]; };
    for (int i = 0; i < n_pts[qi]; ++i) {
      const V3 c = cam_point(st), w = to_world(P, c);
      double o[2];
      pix(i % 3 == 0 && n_pts[qi] != 3 ? cam_point(st) : c, o);  // every third match is wrong, but for a query of exactly three
      Q.p3.insert(Q.p3.end(), w.v, w.v + 3); Q.p2.insert(Q.p2.end(), o, o + 2);
    }
    const int n_l3 = (n_seg[qi] + 1) / 2;  // two segments per 3D line
    std::vector<V3> ea, eb;
    for (int i = 0; i < n_l3; ++i) {
      V3 a = cam_point(st), b = cam_point(st);
      ea.push_back(a); eb.push_back(b);
      const V3 A = to_world(P, a), B = to_world(P, b);
      Q.l3.insert(Q.l3.end(), A.v, A.v + 3); Q.l3.insert(Q.l3.end(), B.v, B.v + 3);
    }
    for (int i = 0; i < n_seg[qi]; ++i) {
      double o[4];
      pix(i % 4 == 0 ? cam_point(st) : ea[(size_t)(i % n_l3)], o);
      pix(eb[(size_t)(i % n_l3)], o + 2);
      Q.sg.insert(Q.sg.end(), o, o + 4);
      Q.ids.push_back(i % n_l3);
    }
    Q.po.push_back((int64_t)Q.p3.size() / 3); Q.lo.push_back((int64_t)Q.l3.size() / 6); Q.so.push_back((int64_t)Q.sg.size() / 4);
  }
  return Q;
}
// lt_fn_est_host on Q with exact-size outputs; an array without data is a null pointer
int run_loop(const Queries &Q, const lt_est_config &cfg, int64_t cap, int threads, std::vector<double> &pose, std::vector<double> &ds,
             std::vector<int32_t> &is, std::vector<int32_t> &inl, std::vector<double> &tr) {
  const size_t n = (size_t)Q.n();
  pose.assign(7 * n, -1.0); ds.assign(3 * n, -1.0); is.assign(12 * n, -1);
  inl.assign((size_t)Q.N(), -1); tr.assign(n * (size_t)cap * LT_EST_TRACE_DOUBLES, -1.0);
  auto dp = [](const std::vector<double> &v) { return v.empty() ? nullptr : v.data(); };
  return lt_fn_est_host(Q.n(), Q.k.data(), Q.q.data(), Q.t.data(), Q.po.data(), dp(Q.p3), dp(Q.p2), Q.lo.data(), dp(Q.l3), Q.so.data(),
                        Q.ids.empty() ? nullptr : Q.ids.data(), dp(Q.sg), &cfg, cap, threads, pose.data(), ds.data(), is.data(),
                        inl.empty() ? nullptr : inl.data(), tr.empty() ? nullptr : tr.data());
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
    const Queries QS = make_queries({14, 1, 30}, {9, 1, 40}, 99u);
    const std::vector<double> &k = QS.k, &q = QS.q, &t = QS.t, &p3 = QS.p3, &p2 = QS.p2, &l3 = QS.l3, &sg = QS.sg;
    const std::vector<int64_t> &po = QS.po, &lo = QS.lo, &so = QS.so;
    std::vector<int32_t> ids = QS.ids;
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
    // a points-only, a lines-only and a three-point query in one batch: empty types, null arrays where a call has no
    // data of a kind, local optimisations whose every step is skipped
    {
      cfg.round_size = 64;
      std::vector<double> pose, ds, tr;
      std::vector<int32_t> is, inl;
      const Queries M = make_queries({24, 0, 3}, {0, 22, 0}, 7u);
      EXPECT(run_loop(M, cfg, cap, 2, pose, ds, is, inl, tr) == LT_OK && all_finite(pose) && all_finite(ds));
      for (int qi = 0; qi < 3; ++qi) EXPECT(is[(size_t)(12 * qi + 10)] == 1 && is[(size_t)(12 * qi)] >= 99);
      EXPECT(ds[2] == 0.0 && ds[1] > 0.0 && is[9] == 0 && is[8] >= 8);                 // points only: no line ratio
      EXPECT(ds[3 + 1] == 0.0 && ds[3 + 2] > 0.0 && is[12 + 8] == 0 && is[12 + 9] >= 8);  // lines only
      EXPECT(is[24 + 5] == 3 && is[24 + 7] >= 1 && is[24 + 2] + is[24 + 3] + is[24 + 4] == 0);  // three points: p3p alone
      for (int only : {0, 1}) {  // each of the two alone: the other type's arrays are null
        const Queries S = only == 0 ? make_queries({24}, {0}, 8u) : make_queries({0}, {22}, 9u);
        EXPECT(run_loop(S, cfg, cap, 1, pose, ds, is, inl, tr) == LT_OK && all_finite(pose) && is[10] == 1 && is[5] >= 8);
      }
      // a 3D cost with a robust loss in the refinements
      lt_est_config c3 = cfg;
      c3.loc.cost_function = 4;  // E3DLineLineDist2
      c3.loc.loss = 3;           // CauchyLoss
      c3.loc.loss_a = 0.05;
      c3.squared_inlier_thresholds[0] = c3.squared_inlier_thresholds[1] = 0.01;
      EXPECT(run_loop(QS, c3, cap, 2, pose, ds, is, inl, tr) == LT_OK && all_finite(pose) && is[10] == 1 && is[24 + 10] == 1);
      EXPECT(is[7] >= 1 && is[24 + 7] >= 1 && is[5] >= 8 && is[24 + 5] >= 30);
    }
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
