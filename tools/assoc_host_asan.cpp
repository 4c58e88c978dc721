// assoc_host_asan.cpp -- the host twin of the global point-line association (lt_fn_assoc_host, lt_fn_assoc_eval,
// lt_fn_assoc_pcg, lt_fn_assoc_link2d of lt_assoc.cpp) under AddressSanitizer and UBSan, as a program of its own:
// lt_assoc.cpp is compiled into it with LT_HOST_ONLY and the sanitizers; nothing is loaded into Python and no device
// is touched.  `make -C limap_amd/csrc assoc_asan` builds and runs it.
// The cases: a scene of 4 cameras with points on lines along three orthogonal directions, three vanishing points and
// every edge kind; every switch; the traced solve; the zero-gradient end and the no-residual end; the refusals; the
// evaluation with all of its outputs; the linear solve at 1, 255, 256 and 257 unknowns, a breakdown and a bad pivot.
// Every array is exactly as long as the call may read or write.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

bool has(const char *what) { return host_asan::has(lt_fn_assoc_host_error, what); }

struct Scene : Cameras {
  std::vector<int32_t> pimg, limg, ek, ea, eb;
  std::vector<double> p3, pxy, line6, l2d, vp, ew;
  std::vector<int64_t> poff{0}, loff{0};
  lt_assoc_input input() const {
    lt_assoc_input in{};
    in.n_img = (int32_t)ids.size();
    in.img_ids = ids.data(); in.kvec4 = k.data(); in.qvec4 = q.data(); in.tvec3 = t.data();
    in.n_pt = (int64_t)poff.size() - 1;
    in.pt3 = p3.data(); in.pt_off = poff.data(); in.pt_img = pimg.data(); in.pt_xy2 = pxy.data();
    in.n_ln = (int64_t)loff.size() - 1;
    in.line6 = line6.data(); in.ln_off = loff.data(); in.ln_img = limg.data(); in.l2d4 = l2d.data();
    in.n_vp = (int64_t)vp.size() / 3;
    in.vp3 = vp.data();
    in.n_edge = (int64_t)ek.size();
    in.edge_kind = ek.data(); in.edge_a = ea.data(); in.edge_b = eb.data(); in.edge_w = ew.data();
    return in;
  }
};

Scene make(int n_cams, int lines_per_dir, unsigned seed) {
  Scene s;
  unsigned st = seed;
  camera_row(s, n_cams);
  int n_lines = 0, n_points = 0;
  for (int dir = 0; dir < 3; ++dir)
    for (int l = 0; l < lines_per_dir; ++l, ++n_lines) {
      double a[3] = {jitter(st), jitter(st), jitter(st)}, b[3] = {a[0], a[1], a[2]};
      b[dir] += 1.2;
      for (int c = 0; c < n_cams; ++c) {
        double xa[2], xb[2];
        s.limg.push_back(s.ids[(size_t)((c + n_lines) % n_cams)]);
        project(s, (c + n_lines) % n_cams, a, xa);
        project(s, (c + n_lines) % n_cams, b, xb);
        const double seg[4] = {xa[0] + 0.3 * jitter(st), xa[1] + 0.3 * jitter(st), xb[0] + 0.3 * jitter(st), xb[1] + 0.3 * jitter(st)};
        s.l2d.insert(s.l2d.end(), seg, seg + 4);
      }
      s.loff.push_back((int64_t)s.limg.size());
      for (int x = 0; x < 3; ++x) s.line6.push_back(a[x] + 0.02 * jitter(st));
      for (int x = 0; x < 3; ++x) s.line6.push_back(b[x] + 0.02 * jitter(st));
      for (int p = 0; p < 2; ++p, ++n_points) {  // two points on the line
        double X[3] = {a[0], a[1], a[2]};
        X[dir] += 0.3 + 0.5 * p;
        for (int c = 0; c < n_cams; ++c) {
          double xy[2];
          project(s, c, X, xy);
          s.pimg.push_back(s.ids[(size_t)c]);
          s.pxy.push_back(xy[0] + 0.3 * jitter(st));
          s.pxy.push_back(xy[1] + 0.3 * jitter(st));
        }
        s.poff.push_back((int64_t)s.pimg.size());
        for (int x = 0; x < 3; ++x) s.p3.push_back(X[x] + 0.02 * jitter(st));
        s.ek.push_back(0); s.ea.push_back(n_points); s.eb.push_back(n_lines); s.ew.push_back(4.0);
      }
      s.ek.push_back(1); s.ea.push_back(dir); s.eb.push_back(n_lines); s.ew.push_back(4.0);
    }
  for (int dir = 0; dir < 3; ++dir)
    for (int x = 0; x < 3; ++x) s.vp.push_back((x == dir ? 1.0 : 0.0) + 0.03 * jitter(st));
  const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (const auto &pr : pairs) { s.ek.push_back(2); s.ea.push_back(pr[0]); s.eb.push_back(pr[1]); s.ew.push_back(1.0); }
  s.ek.push_back(3); s.ea.push_back(0); s.eb.push_back(1); s.ew.push_back(1.0);
  return s;
}

struct Out {
  std::vector<double> pts, params, vps;
  double cost[2] = {0, 0};
  int32_t iters = -1, code = -1;
  int64_t cg = -1;
};

int solve(const Scene &s, const lt_assoc_config &cfg, int threads, Out &o, int64_t cap = 0, std::vector<double> *rec = nullptr,
          int64_t *n = nullptr, double *total0 = nullptr) {
  const lt_assoc_input in = s.input();
  o.pts.assign(3 * (size_t)in.n_pt, 0.0);
  o.params.assign(6 * (size_t)in.n_ln, 0.0);
  o.vps.assign(3 * (size_t)in.n_vp, 0.0);
  if (rec) rec->assign(6 * (size_t)cap, 0.0);
  return lt_fn_assoc_host(&in, &cfg, threads, o.pts.data(), o.params.data(), o.vps.data(), o.cost, &o.iters, &o.cg, &o.code, cap, n,
                          total0, rec ? rec->data() : nullptr);
}

void pcg_case(int n, bool indefinite, bool bad_pivot) {
  unsigned st = 77u + (unsigned)n;
  std::vector<int32_t> nd((size_t)n), ea, eb;
  std::vector<double> diag(16 * (size_t)n, 0.0), rhs(4 * (size_t)n), off;
  for (int u = 0; u < n; ++u) {
    nd[(size_t)u] = u % 5 == 4 ? 0 : 2 + u % 3;
    for (int i = 0; i < 4; ++i) {
      diag[16 * (size_t)u + 5 * i] = 6.0 + jitter(st);
      rhs[4 * (size_t)u + i] = jitter(st);
    }
  }
  for (int u = 0; u + 1 < n; u += 2) {
    ea.push_back(u); eb.push_back((u + 1 + (u % 7)) % n == u ? u + 1 : (u + 1 + (u % 7)) % n);
    for (int i = 0; i < 16; ++i) off.push_back((indefinite ? 40.0 : 0.3) * jitter(st));
  }
  if (bad_pivot) diag[0] = -1.0;
  std::vector<double> x(4 * (size_t)n, -1.0);
  int32_t it = -1, end = -1;
  double rz[2];
  const int rc = lt_fn_assoc_pcg(n, nd.data(), diag.data(), (int64_t)ea.size(), ea.data(), eb.data(), off.data(), rhs.data(), 1e-10, 100,
                                 x.data(), &it, &end, rz);
  EXPECT(rc == LT_OK);
  if (bad_pivot) EXPECT(end == 3 && it == 0);
  else if (indefinite) EXPECT(end == 2);
  else EXPECT(end == 0 && it >= 1 && rz[1] <= rz[0]);
}

}  // namespace

int main() {
  lt_assoc_config cfg;
  lt_assoc_config_default(&cfg);
  EXPECT(cfg.cg_eta == 0.1 && cfg.cg_max_iterations == 500 && cfg.constant_pose == 1);
  const Scene s = make(4, 2, 1);
  Out a, b;
  cfg.max_num_iterations = 25;
  cfg.lw_vp_collinearity = 0.5;
  EXPECT(solve(s, cfg, 1, a) == LT_OK && a.cost[1] < a.cost[0] && a.iters == 25 && a.cg >= 25);
  EXPECT(solve(s, cfg, 3, b) == LT_OK && a.pts == b.pts && a.params == b.params && a.vps == b.vps && a.cg == b.cg);
  // the traced solve
  std::vector<double> rec;
  int64_t n_att = 0;
  double total0 = 0.0;
  EXPECT(solve(s, cfg, 2, b, 8, &rec, &n_att, &total0) == LT_OK && n_att == 25 && 0.5 * total0 == b.cost[0] && rec[0] == 1e4);
  // every switch
  for (int m = 0; m < 64; ++m) {
    lt_assoc_config c = cfg;
    c.max_num_iterations = 4;
    c.constant_point = m & 1; c.constant_line = (m >> 1) & 1; c.constant_vp = (m >> 2) & 1;
    c.enable_pointline = (m >> 3) & 1; c.enable_vpline = (m >> 4) & 1;
    c.lw_point = (m >> 5) & 1 ? 0.0 : 0.1;
    Out o;
    EXPECT(solve(s, c, 2, o) == LT_OK && (o.code == 0 || o.code == 2 || o.code == 7));
    if (c.constant_point) EXPECT(o.pts == s.p3);
  }
  // the evaluation with all of its outputs
  {
    const lt_assoc_input in = s.input();
    int64_t dims[8];
    EXPECT(lt_fn_assoc_eval(&in, &cfg, nullptr, dims, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr) == LT_OK);
    const size_t NU = (size_t)dims[0], NB = (size_t)dims[4], NE = (size_t)dims[5];
    EXPECT(NU == 12 + 6 + 3 && NE == s.ek.size());
    std::vector<int32_t> nd(NU), bu(NB), ei(3 * NE);
    std::vector<double> ew(NE), sp(6 * NU), rb(2 * NB), re(3 * NE), g(4 * NU), dg(16 * NU), of(16 * NE);
    double cost = -1.0;
    EXPECT(lt_fn_assoc_eval(&in, &cfg, nullptr, dims, nd.data(), bu.data(), ei.data(), ew.data(), sp.data(), rb.data(), re.data(), &cost,
                            g.data(), dg.data(), of.data()) == LT_OK);
    EXPECT(cost == a.cost[0]);
    EXPECT(lt_fn_assoc_eval(&in, &cfg, sp.data(), dims, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &cost, nullptr,
                            nullptr, nullptr) == LT_OK && cost == a.cost[0]);
  }
  // the early ends
  {
    lt_assoc_config c = cfg;
    c.constant_point = c.constant_line = c.constant_vp = 1;
    Out o;
    EXPECT(solve(s, c, 2, o) == LT_OK && o.code == 7 && o.iters == 0);
    Scene z = s;
    z.vp = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    c = cfg;
    c.constant_point = c.constant_line = 1; c.enable_pointline = 0; c.lw_vpline_association = 0.0; c.lw_vp_collinearity = 0.0;
    EXPECT(solve(z, c, 2, o) == LT_OK && o.code == 2 && o.iters == 0 && o.vps == z.vp);
  }
  // the refusals
  {
    Out o;
    lt_assoc_config c = cfg;
    c.constant_pose = 0;
    EXPECT(solve(s, c, 1, o) == LT_ERR_ARGUMENT && has("constant_pose"));
    c = cfg; c.constant_intrinsics = 0;
    EXPECT(solve(s, c, 1, o) == LT_ERR_ARGUMENT && has("constant_intrinsics"));
    Scene z = s;
    z.vp[3] = z.vp[4] = z.vp[5] = 0.0;
    EXPECT(solve(z, cfg, 1, o) == LT_ERR_ARGUMENT && has("zero length"));
    z = s; z.p3[1] = std::nan("");
    EXPECT(solve(z, cfg, 1, o) == LT_ERR_ARGUMENT && has("non-finite"));
    z = s; z.ea[0] = 1000;
    EXPECT(solve(z, cfg, 1, o) == LT_ERR_ARGUMENT && has("not in the collection"));
    z = s; z.limg[0] = 4;
    EXPECT(solve(z, cfg, 1, o) == LT_ERR_ARGUMENT && has("not in the collection"));
  }
  for (int n : {1, 255, 256, 257}) pcg_case(n, false, false);
  pcg_case(12, true, false);
  pcg_case(12, false, true);
  const double l1[4] = {0, 0, 100, 0}, l2[4] = {10, 1, 90, 2}, l3[4] = {10, 40, 90, 41};
  EXPECT(lt_fn_assoc_link2d(l1, l2) == 1 && lt_fn_assoc_link2d(l1, l3) == 0);
  return finish("assoc_host_asan");
}
