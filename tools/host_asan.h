// host_asan.h -- the harness the sanitizer programs of tools/*_host_asan.cpp share: the failure counter and EXPECT, the
// final line, the search in a unit's error text, the deterministic noise, and the camera row of the bundle adjustment's
// and the association's scenes.  A new program includes this and keeps only its own cases.
#pragma once

#include "../include/limap_amd.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace host_asan {

inline int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++host_asan::failures;                                          \
    }                                                                 \
  } while (0)

// the program's last statement: the success line only when no EXPECT failed; main's exit code
inline int finish(const char *name) {
  if (failures == 0) std::printf("%s: all checks passed\n", name);
  else std::printf("%s: %d check(s) FAILED\n", name, failures);
  return failures == 0 ? 0 : 1;
}

// whether the text behind a unit's error getter (lt_fn_*_host_error) holds `what`
inline bool has(const char *(*getter)(void), const char *what) { return std::string(getter()).find(what) != std::string::npos; }

// a deterministic stand-in for noise in [-1, 1)
inline double jitter(unsigned &state) {
  state = state * 1664525u + 1013904223u;
  return (double)(state >> 8) / 8388608.0 - 1.0;
}

// cameras in a row looking down +z from z = -5, slightly turned about y; structure around the origin
struct Cameras {
  std::vector<int32_t> ids;
  std::vector<double> k, q, t;
};

inline void camera_row(Cameras &s, int n_cams) {
  for (int c = 0; c < n_cams; ++c) {
    s.ids.push_back(5 + 3 * c);
    const double kk[4] = {600, 590, 400, 300};
    s.k.insert(s.k.end(), kk, kk + 4);
    const double a = 0.05 * (c - 0.5 * n_cams);
    const double qq[4] = {std::cos(a), 0.0, std::sin(a), 0.0};
    s.q.insert(s.q.end(), qq, qq + 4);
    const double tt[3] = {0.8 * (c - 0.5 * n_cams), 0.1 * c, 5.0};
    s.t.insert(s.t.end(), tt, tt + 3);
  }
}

inline void project(const Cameras &s, int c, const double X[3], double xy[2]) {
  // the turn is small: the rotation of the unit quaternion (w, 0, y, 0)
  const double w = s.q[4 * c], y = s.q[4 * c + 2], n = w * w + y * y;
  const double r00 = (w * w - y * y) / n, r02 = 2 * w * y / n, r20 = -r02, r22 = r00;
  const double x = r00 * X[0] + r02 * X[2] + s.t[3 * c], yy = X[1] + s.t[3 * c + 1], z = r20 * X[0] + r22 * X[2] + s.t[3 * c + 2];
  xy[0] = s.k[4 * c] * x / z + s.k[4 * c + 2];
  xy[1] = s.k[4 * c + 1] * yy / z + s.k[4 * c + 3];
}

}  // namespace host_asan

using namespace host_asan;
