// lt_twin.h -- what the entry points of a host twin share (lt_fn_*_host, lt_fn_*_eval: the kernels' inline functions run on
// the CPU): the per-thread error slot behind a unit's lt_fn_*_host_error and the unpacking of a minimiser's packed sums.
// Host only: nothing beyond the standard library and the C ABI, so a unit compiled with LT_HOST_ONLY (no context, no HIP
// runtime: the sanitizer programs of tools/*_host_asan.cpp) includes it as it stands.  A new twin uses these, it does not
// bring its own.
#pragma once

#include "../../include/limap_amd.h"

#include <algorithm>
#include <string>

namespace lt_impl {

// The error text of a unit's host entry points: one thread_local object per unit, read by the unit's public getter.
struct HostError {
  std::string text;
  // "who: msg" into the slot; the refusal's code back
  int refuse(const char *who, const std::string &msg) {
    text = std::string(who) + ": " + msg;
    return LT_ERR_ARGUMENT;
  }
  // an entry point's opening check (`failed` usually make_plan(..., msg)): the refusal, or LT_OK and an empty slot
  int check(const char *who, bool failed, const std::string &msg) {
    if (failed) return refuse(who, msg);
    text.clear();
    return LT_OK;
  }
  void clear() { text.clear(); }
  const char *c_str() const { return text.c_str(); }
};

// The packed sums of a linearisation (lm_step's layout): the upper triangle of the N x N matrix row by row, then the N
// entries of the gradient.  Either output may be null.
template <int N>
inline void sums_to_gH(const double *acc, double *g, double *H) {
  constexpr int kTri = N * (N + 1) / 2;
  if (H) {
    int o = 0;
    for (int i = 0; i < N; ++i)
      for (int j = i; j < N; ++j, ++o) H[N * i + j] = H[N * j + i] = acc[o];
  }
  if (g) std::copy(acc + kTri, acc + kTri + N, g);
}

}  // namespace lt_impl
