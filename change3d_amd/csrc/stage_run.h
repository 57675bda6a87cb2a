// How the residual-stage driver runs a launch: the per-launch profiler and the side stream.
// The state below (g_prof*, g_side, g_mu) is per process and must exist ONCE: this header is included by stage_driver.hip
// alone.  Should a second translation unit need it, the definitions move into one .hip first.
#pragma once
#include "../../include/change3d_hip.h"
#include <hip/hip_runtime.h>
#include "common.h"
#include "launch_hints.h"
#include "stage_plan.h"   // es()
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <vector>

namespace {

#define RC(call)              \
  do {                        \
    const int rc_ = (call);   \
    if (rc_ != 0) return rc_; \
  } while (0)
#define HIPRC(call)                            \
  do {                                         \
    const hipError_t e_ = (call);              \
    if (e_ != hipSuccess) return (int)e_;      \
  } while (0)

// ------------------------------------------------------------------------------------------ per-launch profile
// c3d_prof_begin / c3d_prof_end (include/change3d_hip.h): every kernel the driver enqueues is bracketed by a HIP event
// pair on the stream it is launched on and billed its algorithmic bytes, so bench.py's per-kernel table and `roofline`
// block are taken through THIS launch sequence (round 2 took them through a second, Python, copy of it).
struct ProfRec { char name[64]; hipEvent_t e0, e1; double bytes; };
std::vector<ProfRec> g_prof;
int g_prof_flags = -1;   // < 0: off; bit 0: weight gradients inline on the main stream; bit 1: names carry shape / mode
char g_prof_tag[32] = "";   // detail mode: geometry of the block being enqueued, appended to names without a shape of their own

template <typename F>
int prof_call(const char* name, double bytes, hipStream_t s, F&& fn) {
  if (g_prof_flags < 0) return fn();
  ProfRec r;
  if ((g_prof_flags & 2) && g_prof_tag[0] && !std::strchr(name, '['))
    std::snprintf(r.name, sizeof(r.name), "%s[%s]", name, g_prof_tag);
  else
    std::snprintf(r.name, sizeof(r.name), "%s", name);
  r.bytes = bytes;
  HIPRC(hipEventCreate(&r.e0));
  HIPRC(hipEventCreate(&r.e1));
  HIPRC(hipEventRecord(r.e0, s));
  const int rc = fn();
  HIPRC(hipEventRecord(r.e1, s));
  g_prof.push_back(r);
  return rc;
}
inline bool prof_detail() { return g_prof_flags >= 0 && (g_prof_flags & 2); }

// detail mode: the rows of the block being enqueued carry its geometry (both training passes, at the top of every block)
inline void prof_tag_block(int H, int Ci, int s, bool se) {
  if (prof_detail()) std::snprintf(g_prof_tag, sizeof(g_prof_tag), "H=%d Ci=%d s=%d se=%d", H, Ci, s, (int)se);
}

// profile row of a pointwise GEMM launch, whichever entry point `fn` takes
template <typename F>
int pw_prof(const c3d_pw_args& a, hipStream_t st, F&& fn) {
  const double bytes = (double)a.M * ((double)a.Kp * (a.x2 ? 2 : 1) + (double)a.Np * (a.e1 ? 2 : 1) + (a.pro_out ? a.Kp : 0) +
                                     ((a.wg_mode == C3D_WG_ROWS || a.wg_mode == C3D_WG_MASKSUM) ? a.Np : 0) + (a.add_sums ? a.Np : 0)) * (double)es(a.dtype);
  char nm[64];
  if (prof_detail())
    std::snprintf(nm, sizeof(nm), "c3d_pw_gemm[M=%lld K=%d N=%d pro=%d epi=%d rows=%d%s]", (long long)a.M, a.K, a.N, a.pro_mode,
                  a.epi_mode, a.row_mode, a.wg_mode == C3D_WG_MASKSUM ? " +bob" : a.wg_mode ? (a.add_sums ? " +dW +bob" : " +dW") : "");
  else
    std::snprintf(nm, sizeof(nm), "c3d_pw_gemm");
  return prof_call(nm, bytes, st, fn);
}

inline int pw_launch(const c3d_pw_args& a, hipStream_t st) {
  return pw_prof(a, st, [&] { return c3d_pw_gemm(&a, st); });
}

inline int wg_launch(const c3d_pw_wgrad_args& a, hipStream_t st) {
  const double bytes = (double)a.M * ((double)a.Np * (a.p2 ? 2 : 1) + (double)a.Kp) * (double)es(a.dtype);
  char nm[64];
  if (prof_detail())
    std::snprintf(nm, sizeof(nm), "c3d_pw_wgrad[M=%lld K=%d N=%d q=%d rows=%d]", (long long)a.M, a.K, a.N, a.q_mode, a.row_mode);
  else
    std::snprintf(nm, sizeof(nm), "c3d_pw_wgrad");
  return prof_call(nm, bytes, st, [&] { return c3d_pw_wgrad(&a, st); });
}

// ------------------------------------------------------------------------------------------ side stream
struct SideCtx {
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> pool;
  size_t next = 0;
  std::deque<std::pair<uint64_t, hipEvent_t>> marks;   // (sequence, done event) of side work not yet joined
  uint64_t seq = 0;
  hipEvent_t ev() {
    if (pool.size() < 256) {
      hipEvent_t e;
      // fork / done marks between two streams of ONE device: no timing, and no system-scope fence -- the default event makes
      // the recording queue write its caches back for the host and for peer devices at every mark (7-10 us of main-queue
      // bubble per fork in the round-5 trace, two forks per residual block); what leaves the device (the gradient all-reduce,
      // the host reading the loss) is ordered by the caller's own events / synchronisation behind c3d_side_join
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return nullptr;
      pool.push_back(e);
      return e;
    }
    next = (next + 1) % pool.size();
    return pool[next];
  }
};

std::mutex g_mu;
SideCtx g_side[16];

// The side stream is on unless C3D_OPT_SIDE_STREAM turned it off or a profile asked for serial launches
// (c3d_prof_begin flags bit 0).  The second clause reaches further than the weight gradients, on purpose: coop_launch
// (stage_driver.hip) defers its reducers to the end of the pass only while this holds, and a serial profile therefore
// sees slot 0 and the reducer right behind each cooperative kernel.
inline bool side_enabled() { return c3d_option_side_stream != 0 && !(g_prof_flags >= 0 && (g_prof_flags & 1)); }

inline SideCtx* side_ctx() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  SideCtx& c = g_side[dev];
  if (!c.side) {
    // C3D_SIDE_PRIO=1: lowest stream priority for the weight-gradient stream (A/B knob)
    static const bool low = c3d_env("C3D_SIDE_PRIO") && atoi(c3d_env("C3D_SIDE_PRIO")) == 1;
    int lo = 0, hi = 0;
    if (low && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) {
      if (hipStreamCreateWithPriority(&c.side, hipStreamNonBlocking, lo) != hipSuccess) return nullptr;
    } else if (hipStreamCreateWithFlags(&c.side, hipStreamNonBlocking) != hipSuccess) {
      return nullptr;
    }
  }
  return &c;
}

// Run `fn(stream)` on the side stream after everything issued so far on `main` (inline when disabled).
template <typename F>
int side_run(hipStream_t main, F&& fn) {
  if (!side_enabled()) return fn(main);
  std::lock_guard<std::mutex> lk(g_mu);
  SideCtx* c = side_ctx();
  if (!c) return fn(main);
  hipEvent_t fork = c->ev();
  if (!fork) return fn(main);
  HIPRC(hipEventRecord(fork, main));
  HIPRC(hipStreamWaitEvent(c->side, fork, 0));
  c3d_side_launch = 1;           // launch hint (launch_hints.h): this kernel runs beside the data-gradient chain
  const int rc_fn = fn(c->side);
  c3d_side_launch = 0;
  RC(rc_fn);
  hipEvent_t done = c->ev();
  if (!done) return (int)hipErrorOutOfMemory;
  HIPRC(hipEventRecord(done, c->side));
  c->marks.emplace_back(++c->seq, done);
  while (c->marks.size() > 64) c->marks.pop_front();   // older work is ordered before the newer marks on the side stream
  return 0;
}

inline uint64_t side_mark() {
  std::lock_guard<std::mutex> lk(g_mu);
  SideCtx* c = side_ctx();
  return c ? c->seq : 0;
}

// `main` waits for the side work issued up to sequence `upto` (everything if upto == UINT64_MAX).
inline int side_join(hipStream_t main, uint64_t upto) {
  std::lock_guard<std::mutex> lk(g_mu);
  SideCtx* c = side_ctx();
  if (!c) return 0;
  hipEvent_t last = nullptr;
  while (!c->marks.empty() && c->marks.front().first <= upto) {
    last = c->marks.front().second;
    c->marks.pop_front();
  }
  if (last) HIPRC(hipStreamWaitEvent(main, last, 0));
  return 0;
}

}  // namespace
