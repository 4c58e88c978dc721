// lt_hostutil.h -- the host toolkit of the modules around the triangulation core (lt_merge, lt_fit, lt_eval, lt_bpt,
// lt_match, lt_vp, lt_refine, lt_sfm, the remerge of lt_tracks): stream synchronisation, HIP event timing, transfers of host
// vectors, input checks, the counted-output launch loop and the polled loop of the coupled solves.  A new module uses
// these, it does not bring its own.  Included from lt_host.h.  What a host twin's entry points share without
// a context or the HIP runtime (the error slot, the unpacking of the packed sums) is lt_twin.h.
#pragma once

#include "lt_ctx.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace lt_impl {

// waits for the context's stream and picks up the error of any launch before it
inline int stream_sync(lt_ctx *ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipGetLastError());
  return LT_OK;
}

// The HIP events of one call, destroyed on every return path; their count is chosen at run time (EventList) or fixed
// (Events<N>).  ms(a, b) is 0 unless both events were recorded (and the stream has passed them: callers synchronise
// first).  A launch wrapper that records the events itself takes data(); its caller then says mark_all().
struct EventList {
  std::vector<hipEvent_t> e;
  std::vector<char> recorded;
  explicit EventList(int n) : e((size_t)n, nullptr), recorded((size_t)n, 0) {}
  EventList(const EventList &) = delete;
  EventList &operator=(const EventList &) = delete;
  ~EventList() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int size() const { return (int)e.size(); }
  hipEvent_t *data() { return e.data(); }
  int create(lt_ctx *ctx) {
    for (hipEvent_t &x : e) HIPCHK(ctx, hipEventCreate(&x));
    return LT_OK;
  }
  int record(lt_ctx *ctx, int k) {
    HIPCHK(ctx, hipEventRecord(e[(size_t)k], ctx->stream));
    recorded[(size_t)k] = 1;
    return LT_OK;
  }
  void mark_all() { recorded.assign(recorded.size(), 1); }
  double ms(int a, int b) const {
    float v = 0.f;
    if (!recorded[(size_t)a] || !recorded[(size_t)b] || hipEventElapsedTime(&v, e[(size_t)a], e[(size_t)b]) != hipSuccess) return 0.0;
    return v;
  }
};
template <int N>
struct Events : EventList {
  Events() : EventList(N) {}
};

template <class T>
int upload_vec(lt_ctx *ctx, DevBuf &buf, const std::vector<T> &v) {
  ENSURE(ctx, buf, sizeof(T) * std::max<size_t>(v.size(), 1));
  if (!v.empty())
    HIPCHK(ctx, hipMemcpyAsync(buf.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, ctx->stream));
  return LT_OK;
}

// n items of device memory into dst (resized), on the context's stream: complete after the next stream_sync
template <class T>
int download(lt_ctx *ctx, std::vector<T> &dst, const void *src, size_t n) {
  dst.resize(n);
  if (n) HIPCHK(ctx, hipMemcpyAsync(dst.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost, ctx->stream));
  return LT_OK;
}

inline bool all_finite(const double *v, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

inline bool all_finite(const float *v, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

inline int check_finite(lt_ctx *ctx, const char *who, const double *v, long long n, const char *what) {
  return all_finite(v, n) ? LT_OK : fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": non-finite " + what);
}

// what is wrong with the CSR offsets off[0 .. n] of the `what`s ("line", "point", ...); empty when nothing is
inline std::string offsets_msg(const char *what, long long n, const int64_t *off) {
  if (!off) return std::string("null ") + what + " offsets";
  if (off[0] != 0) return std::string(what) + " offsets must start at 0";
  for (long long k = 0; k < n; ++k)
    if (off[k + 1] < off[k]) return std::string(what) + " offsets decrease";
  return std::string();
}

inline int check_offsets(lt_ctx *ctx, const char *who, const char *what, long long n, const int64_t *off) {
  const std::string msg = offsets_msg(what, n, off);
  return msg.empty() ? LT_OK : fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": " + msg);
}

// The counted-output launch: buf = [counter (8 B) padded to `head` bytes | capacity items of `item` bytes].
// launch(items, capacity, counter) enqueues kernels that count every item they find and store those that fit; it
// returns LT_OK or an error code.  A launch that counted more than it had room for runs again with room for all of
// them, so a deterministic kernel needs two attempts at most and the bound of 8 is only a guard.  With peek > 0 the
// counter and the first `peek` items come back in ONE copy of head + peek * item bytes into peek_dst (a second copy
// behind the first costs a remerge pass a round trip).  Leaves the stream idle.
template <class Launch>
int run_counted(lt_ctx *ctx, DevBuf &buf, size_t head, size_t item, unsigned long long capacity, Launch launch,
                unsigned long long *count, int *attempts, void *peek_dst = nullptr, size_t peek = 0) {
  hipStream_t st = ctx->stream;
  for (*attempts = 1; *attempts <= 8; ++*attempts) {
    ENSURE(ctx, buf, head + item * (size_t)std::max<unsigned long long>(capacity, peek));
    HIPCHK(ctx, hipMemsetAsync(buf.p, 0, 8, st));
    if (int rc = launch(static_cast<void *>(buf.as<char>() + head), capacity, buf.as<unsigned long long>())) return rc;
    HIPCHK(ctx, hipGetLastError());
    unsigned long long n = 0;
    HIPCHK(ctx, hipMemcpyAsync(peek ? peek_dst : &n, buf.p, peek ? head + item * peek : 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (peek) std::memcpy(&n, peek_dst, 8);
    if (n <= capacity) {
      *count = n;
      return LT_OK;
    }
    capacity = n;
  }
  return fail(ctx, LT_ERR_STATE, "k_track_connect: the edge count kept growing between launches");
}

// The polled device loop of a solve whose decisions are made on the device: `poll` times launch() -- one attempt or
// batch, whose kernels return at once when the solve has ended, so the result does not depend on the interval -- then
// the status record comes back in one copy and the stream is synchronised; after() follows every synchronisation (the
// callers add their event times there), and the loop ends when done(status).  *launched counts the calls of launch().
// Nothing is allocated and nothing but the one copy is enqueued here.
template <class Status, class Launch, class Done, class After>
int run_polled(lt_ctx *ctx, int poll, const void *d_status, Status &status, Launch launch, Done done, After after,
               long long *launched) {
  for (*launched = 0;;) {
    for (int k = 0; k < poll; ++k, ++*launched) launch();
    HIPCHK(ctx, hipMemcpyAsync(&status, d_status, sizeof(Status), hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = stream_sync(ctx)) return rc;
    after();
    if (done(status)) return LT_OK;
  }
}

}  // namespace lt_impl
