// vsx_window.h -- the two-slot window pipeline the read commands share (vsx_merge.cpp, vsx_filter.cpp, vsx_eestats.cpp,
// vsx_fastq_stats.cpp): a call cuts its input into windows of consecutive reads; window k + 1 is staged on one slot's stream while
// window k runs on the other's, and the windows are collected in input order.  Host-only C++.  What a window's bytes look like,
// which kernels run on them and what becomes of the results is each command's own: it derives its slot from Slot<> and gives
// run_windows its plan, its submit and its collect.
#ifndef VSX_WINDOW_H
#define VSX_WINDOW_H

#include "vsx_private.h"

namespace vsxp __attribute__((visibility("hidden"))) {

// one of the two windows in flight: a non-blocking stream, the events the command times its stages with (it names the indices),
// and the reads [w0, w0 + n) the slot works on while it is busy.  The command's slot adds the buffers.
template <int EVENTS>
struct Slot {
  hipStream_t st = nullptr;
  hipEvent_t ev[EVENTS] = {};
  uint64_t w0 = 0, n = 0;               // the window in flight
  bool busy = false;
  Slot() = default;
  Slot(const Slot &) = delete;
  Slot & operator=(const Slot &) = delete;
  ~Slot()
  {
    if (st) (void) hipStreamSynchronize(st);
    for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e);
    if (st) (void) hipStreamDestroy(st);
  }
  int create(const char * who)
  {
    VSX_HIP_AS(who, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (hipEvent_t & e : ev) VSX_HIP_AS(who, hipEventCreate(&e));
    return VSX_OK;
  }
  // the device time between two of the slot's events, added to a field of the command's stats
  hipError_t add_elapsed(int from, int to, double & seconds)
  {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, ev[from], ev[to]);
    if (e == hipSuccess) seconds += ms * 1e-3;
    return e;
  }
};

// a pinned staging buffer and its device twin, grown together: replaced (the old pair freed first) by a pair of `want` bytes when
// the device block is missing or holds less than `need`.  How much headroom `want` carries is the caller's policy.
inline int grow_pair(const char * who, PinnedBuf<uint8_t> & h, DevBuf<uint8_t> & d, uint64_t need, uint64_t want)
{
  if (d.p && need <= d.n) return VSX_OK;
  h.release(); d.release();
  VSX_HIP_AS(who, h.alloc(want));
  VSX_HIP_AS(who, d.alloc(want));
  return VSX_OK;
}

// the bytes [lo, hi) of one side's blobs that the reads of a window touch
struct Span { uint64_t lo = 0, hi = 0; };

// what a plan returns: the number of reads of the window, and per side the span it copies (where the command plans by span)
struct Window {
  uint64_t n = 0;
  Span span[2];
};

// where the reads of one side lie in its blobs
struct Side {
  const uint64_t * off;
  const uint32_t * len;
};

// extend the window at w0 greedily: up to `window` reads, every side's span within the capacity; a single read always fits
inline Window plan_window(const Side * side, int n_sides, uint64_t w0, uint64_t n_total, uint64_t window, uint64_t capacity)
{
  Window W;
  for (uint64_t k = w0; k < n_total && W.n < window; ++k, ++W.n)
    {
      Span next[2];
      bool fits = true;
      for (int s = 0; s < n_sides; ++s)
        {
          const uint64_t lo = side[s].off[k], hi = lo + side[s].len[k];
          next[s].lo = W.n ? std::min(W.span[s].lo, lo) : lo;
          next[s].hi = W.n ? std::max(W.span[s].hi, hi) : hi;
          fits = fits && next[s].hi - next[s].lo <= capacity;
        }
      if (W.n && !fits) break;
      W.span[0] = next[0]; W.span[1] = next[1];
    }
  return W;
}

// The driver: for every window, collect what the slot about to be reused still holds, plan, submit, count; then drain.
//   plan(w0) -> Window             the window that starts at read w0 (at least one read)
//   submit(slot, other, w0, W)     stage the window into `slot` and enqueue its work (`other` holds the window before it)
//   collect(slot)                  wait for the slot's window and take its results
// submit and collect return a VSX_ code; anything but VSX_OK ends the call at once, so the first failing read in input order is
// the one that is reported.
template <typename SlotT, typename Plan, typename Submit, typename Collect>
int run_windows(SlotT (&slot)[2], uint64_t n, Plan && plan, Submit && submit, Collect && collect, uint64_t & windows)
{
  int rc = VSX_OK;
  uint64_t w = 0;
  for (uint64_t w0 = 0; w0 < n; ++w)
    {
      SlotT & s = slot[w & 1];
      if (s.busy && (rc = collect(s)) != VSX_OK) return rc;
      const Window W = plan(w0);
      if ((rc = submit(s, slot[(w + 1) & 1], w0, W)) != VSX_OK) return rc;
      ++windows;
      w0 += W.n;
    }
  for (uint64_t d = 0; d < 2; ++d)
    {
      SlotT & s = slot[(w + d) & 1];          // the older window first
      if (s.busy && (rc = collect(s)) != VSX_OK) return rc;
    }
  return VSX_OK;
}

}  // namespace vsxp

#endif
