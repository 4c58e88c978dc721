// ba_host_asan.cpp -- the host twin of the bundle adjustment with free poses (lt_fn_ba_host, lt_fn_ba_eval,
// lt_fn_ba_cholesky of lt_ba.cpp) under AddressSanitizer and UBSan, as a program of its own: lt_ba.cpp is compiled into
// it with LT_HOST_ONLY and the sanitizers; nothing is loaded into Python and no device is touched.
// `make -C limap_amd/csrc ba_asan` builds and runs it.
// The cases follow tests/test_ba_host.py: a hybrid scene of 4 cameras, 24 points and 6 lines; tracks with 1, 15, 16, 17
// and 33 observations (an image then observes a track more than once); an image without observations in the middle of
// the ids; every switch; constant poses (the separated point solves); termination codes 6 and 7; every refusal; the
// evaluation with its dense H and the Schur step;
// the Cholesky recurrence at sizes 1, 6, 7, 64, 65 and 258.  Every array is exactly as long as the call may read.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

bool has(const char *what) { return host_asan::has(lt_fn_ba_host_error, what); }

struct Scene : Cameras {
  std::vector<int32_t> pimg, limg;
  std::vector<double> p3, pxy, line6, l2d, l3d;
  std::vector<int64_t> poff{0}, loff{0};
};

Scene make(int n_cams, int n_points, int n_lines, const std::vector<int> &pobs, const std::vector<int> &lobs, unsigned seed) {
  Scene s;
  unsigned st = seed;
  camera_row(s, n_cams);
  for (int n = 0; n < n_points; ++n) {
    double X[3] = {jitter(st), jitter(st), jitter(st)};
    const int cnt = n < (int)pobs.size() ? pobs[(size_t)n] : n_cams;
    for (int j = 0; j < cnt; ++j) {
      const int c = (n + j) % n_cams;
      double xy[2];
      project(s, c, X, xy);
      s.pimg.push_back(s.ids[(size_t)c]);
      s.pxy.push_back(xy[0] + 0.5 * jitter(st));
      s.pxy.push_back(xy[1] + 0.5 * jitter(st));
    }
    s.poff.push_back((int64_t)s.pimg.size());
    for (int i = 0; i < 3; ++i) s.p3.push_back(X[i] + 0.02 * jitter(st));
  }
  for (int n = 0; n < n_lines; ++n) {
    double A[3] = {jitter(st), jitter(st), jitter(st)}, B[3];
    const double d[3] = {1.0 + 0.3 * jitter(st), 0.5 * jitter(st), 0.4 * jitter(st)};
    for (int i = 0; i < 3; ++i) B[i] = A[i] + d[i];
    const int cnt = n < (int)lobs.size() ? lobs[(size_t)n] : n_cams;
    for (int j = 0; j < cnt; ++j) {
      const int c = (2 * n + 3 * j) % n_cams;
      double a2[2], b2[2];
      project(s, c, A, a2);
      project(s, c, B, b2);
      s.limg.push_back(s.ids[(size_t)c]);
      const double sg[4] = {a2[0] + 0.5 * jitter(st), a2[1] + 0.5 * jitter(st), b2[0] + 0.5 * jitter(st), b2[1] + 0.5 * jitter(st)};
      s.l2d.insert(s.l2d.end(), sg, sg + 4);
      for (int i = 0; i < 3; ++i) s.l3d.push_back(A[i] + 0.01 * jitter(st));
      for (int i = 0; i < 3; ++i) s.l3d.push_back(B[i] + 0.01 * jitter(st));
    }
    s.loff.push_back((int64_t)s.limg.size());
    for (int i = 0; i < 3; ++i) s.line6.push_back(A[i] + 0.02 * jitter(st));
    for (int i = 0; i < 3; ++i) s.line6.push_back(B[i] + 0.02 * jitter(st));
  }
  for (int c = 0; c < n_cams; ++c)  // the poses start beside the truth
    for (int i = 0; i < 3; ++i) s.t[3 * (size_t)c + i] += 0.03 * jitter(st);
  return s;
}

struct Out {
  std::vector<double> q, t, p, params, seg;
  double cost[2];
  int32_t it, code;
};

int run(const Scene &s, const lt_ba_config &cfg, int threads, Out *o) {
  const size_t N = s.ids.size(), NP = s.poff.size() - 1, NL = s.loff.size() - 1;
  o->q.assign(4 * N, 0.0); o->t.assign(3 * N, 0.0); o->p.assign(3 * NP, 0.0); o->params.assign(6 * NL, 0.0); o->seg.assign(6 * NL, 0.0);
  return lt_fn_ba_host((int)N, s.ids.data(), s.k.data(), s.q.data(), s.t.data(), (int64_t)NP, s.p3.data(), s.poff.data(),
                       s.pimg.data(), s.pxy.data(), (int64_t)NL, s.line6.data(), s.loff.data(), s.limg.data(), s.l2d.data(),
                       s.l3d.data(), &cfg, threads, o->q.data(), o->t.data(), o->p.data(), o->params.data(), o->seg.data(),
                       o->cost, &o->it, &o->code);
}

lt_ba_config config(int iters) {
  lt_ba_config c;
  lt_ba_config_default(&c);
  c.max_num_iterations = iters;
  return c;
}

}  // namespace

int main() {
  Out o, o4;
  const Scene hybrid = make(4, 24, 6, {}, {}, 1);
  for (int threads : {1, 4}) {
    lt_ba_config c = config(20);
    EXPECT(run(hybrid, c, threads, &o) == 0 && std::isfinite(o.cost[0]) && o.cost[1] < 0.2 * o.cost[0] && o.it == 20);
  }
  {  // identical bits for 1 and 4 threads
    lt_ba_config c = config(15);
    EXPECT(run(hybrid, c, 1, &o) == 0 && run(hybrid, c, 4, &o4) == 0);
    EXPECT(o.q == o4.q && o.t == o4.t && o.p == o4.p && o.params == o4.params && o.seg == o4.seg && o.cost[1] == o4.cost[1]);
  }
  {  // the group width of the structure sums and its loop; tracks twice in one image
    const Scene s = make(6, 10, 8, {1, 15, 16, 17, 33, 2, 12}, {1, 15, 16, 17, 33, 7}, 2);
    lt_ba_config c = config(10);
    c.min_num_images = 1;
    c.num_outliers_aggregator = 0;
    EXPECT(run(s, c, 2, &o) == 0 && o.cost[1] < o.cost[0]);
  }
  {  // an image without observations in the middle of the ids keeps its pose
    Scene s = make(4, 12, 4, {}, {}, 3);
    s.ids.insert(s.ids.begin() + 2, 9);
    const double kk[4] = {600, 590, 400, 300}, qq[4] = {0.5, -0.5, 0.25, 2.0}, tt[3] = {7, 8, 9};
    s.k.insert(s.k.begin() + 8, kk, kk + 4);
    s.q.insert(s.q.begin() + 8, qq, qq + 4);
    s.t.insert(s.t.begin() + 6, tt, tt + 3);
    EXPECT(run(s, config(10), 2, &o) == 0);
    EXPECT(o.q[8] == 0.5 && o.q[11] == 2.0 && o.t[6] == 7 && o.t[8] == 9);
  }
  for (int sw = 0; sw < 5; ++sw) {  // the switches
    lt_ba_config c = config(8);
    if (sw == 0) c.constant_point = 1;
    if (sw == 1) c.constant_line = 1;
    if (sw == 2) c.min_num_images = 5;
    if (sw == 3) c.lw_point = 0.0;
    if (sw == 4) { c.constant_point = 1; c.constant_line = 1; c.constant_principal_point = 0; }
    EXPECT(run(hybrid, c, 2, &o) == 0 && o.cost[1] < o.cost[0]);
    if (sw == 0 || sw == 3 || sw == 4) EXPECT(o.p == hybrid.p3);
  }
  {  // code 7: no residual block; code 6: a point in a camera's plane
    Scene s = make(3, 5, 0, {}, {}, 4);
    lt_ba_config c = config(8);
    c.lw_point = 0.0;
    EXPECT(run(s, c, 1, &o) == 0 && o.code == 7 && o.it == 0 && o.p == s.p3 && o.q == s.q);
    s.q[0] = 1.0; s.q[2] = 0.0;
    s.t[0] = 0.0; s.t[1] = 0.0; s.t[2] = 5.0;
    s.p3[6] = 0.3; s.p3[7] = 0.2; s.p3[8] = -5.0;
    EXPECT(run(s, config(8), 1, &o) == 0 && o.code == 6 && o.it == 0 && !std::isfinite(o.cost[0]) && o.p == s.p3);
  }
  {  // constant poses: every point track its own solve, the poses kept
    const Scene s = make(6, 9, 0, {1, 15, 16, 17, 33, 2}, {}, 6);
    lt_ba_config c = config(20);
    c.constant_pose = 1;
    for (int threads : {1, 4}) EXPECT(run(s, c, threads, &o) == 0 && o.cost[1] < o.cost[0] && o.q == s.q && o.t == s.t);
    c.constant_point = 1;
    EXPECT(run(s, c, 1, &o) == 0 && o.code == 7 && o.p == s.p3);
  }
  {  // refusals
    lt_ba_config c = config(8);
    c.constant_intrinsics = 0;
    EXPECT(run(hybrid, c, 1, &o) != 0 && has("constant_intrinsics"));
    c = config(8);
    c.constant_pose = 1;
    EXPECT(run(hybrid, c, 1, &o) != 0 && has("constant_pose"));
    Scene s = hybrid;
    s.pimg[3] = 999;
    EXPECT(run(s, config(8), 1, &o) != 0 && has("not in the collection"));
    s = hybrid;
    s.l2d[5] = NAN;
    EXPECT(run(s, config(8), 1, &o) != 0 && has("non-finite"));
    s = hybrid;
    for (int i = 0; i < 3; ++i) s.line6[6 + 3 + i] = s.line6[6 + i];
    EXPECT(run(s, config(8), 1, &o) != 0 && has("zero length"));
    s = hybrid;
    s.ids[1] = s.ids[0];
    EXPECT(run(s, config(8), 1, &o) != 0 && has("appears twice"));
    const Scene big = make(lt_ba_max_images() + 1, lt_ba_max_images() + 1, 0, std::vector<int>((size_t)lt_ba_max_images() + 1, 2), {}, 5);
    EXPECT(run(big, config(2), 1, &o) != 0 && has("LT_BA_MAX_IMAGES"));
    const Scene most = make(lt_ba_max_images(), lt_ba_max_images(), 0, std::vector<int>((size_t)lt_ba_max_images(), 2), {}, 5);
    EXPECT(run(most, config(2), 2, &o) == 0);
  }
  {  // the evaluation: dims, then every output, and the Schur route's step
    const Scene &s = hybrid;
    const lt_ba_config c = config(8);
    int64_t dims[4];
    const size_t N = s.ids.size(), NP = s.poff.size() - 1, NL = s.loff.size() - 1;
    auto eval = [&](int32_t *info, double *res, double *cost, double *g, double *H, double *step) {
      return lt_fn_ba_eval((int)N, s.ids.data(), s.k.data(), s.q.data(), s.t.data(), (int64_t)NP, s.p3.data(), s.poff.data(),
                           s.pimg.data(), s.pxy.data(), (int64_t)NL, s.line6.data(), s.loff.data(), s.limg.data(), s.l2d.data(),
                           s.l3d.data(), &c, nullptr, dims, info, res, cost, g, H, 1e4, step);
    };
    EXPECT(eval(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    EXPECT(dims[0] == 4 && dims[1] == 24 * 4 + 6 * 4 && dims[2] == 24 + 72 + 24 && dims[3] == 30);
    std::vector<int32_t> info(3 * (size_t)dims[1]);
    std::vector<double> res(2 * (size_t)dims[1]), g((size_t)dims[2]), H((size_t)dims[2] * (size_t)dims[2]), step((size_t)dims[2]);
    double cost;
    EXPECT(eval(info.data(), res.data(), &cost, g.data(), H.data(), step.data()) == 0 && std::isfinite(cost) && std::isfinite(step[0]));
  }
  for (int n : {1, 6, 7, 64, 65, 258}) {  // the Cholesky recurrence
    std::vector<double> S((size_t)n * n, 0.0), rhs((size_t)n, 1.0), L((size_t)n * n), x((size_t)n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) S[(size_t)i * n + j] = (i == j ? n + 1.0 : 0.0) + 1.0 / (1.0 + i + j);
    EXPECT(lt_fn_ba_cholesky(n, S.data(), rhs.data(), L.data(), x.data()) == 0 && std::isfinite(x[(size_t)n - 1]));
    EXPECT(lt_fn_ba_cholesky(n, S.data(), nullptr, L.data(), nullptr) == 0);
    S[0] = -1.0;
    EXPECT(lt_fn_ba_cholesky(n, S.data(), rhs.data(), L.data(), x.data()) != 0);
  }
  return finish("ba_host_asan");
}
