// vsx_align_pairs.cpp -- host side of libvsx, the one-call form: one plan, or a pipeline of plans over slices of a large pair list.
// See vsx_context.cpp for the layout of the host layer.
#include "vsx_host_internal.h"

#include <condition_variable>
#include <thread>

using vsxp::fail;
using namespace vsxh;

extern "C" {

int vsx_align_pairs(vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                    const uint32_t * qidx, const uint32_t * tidx, vsx_results * out)
{
  return vsx_align_pairs_filtered(ctx, queries, targets, n_pairs, qidx, tidx, nullptr, out);
}

// one plan: create, run, fetch, destroy
static int align_pairs_single(vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                              const uint32_t * qidx, const uint32_t * tidx, const vsx_filter * filter, vsx_results * out,
                              RankedSink * sink = nullptr)
{
  static const bool timing = std::getenv("VSX_DEBUG_TIMING") != nullptr;
  double t_plan = 0, t_run = 0, t_fetch = 0, t_destroy = 0;
  vsx_plan * pl = nullptr;
  int rc;
  {
    vsxp::Stopwatch sw(t_plan);
    rc = vsx_plan_create(ctx, &pl, queries, targets, n_pairs, qidx, tidx, 0);
    if (rc != VSX_OK) return rc;
    if (filter) rc = vsx_plan_set_filter(pl, filter);
    if (rc == VSX_OK && sink) rc = plan_set_ranked(pl);
    if (rc != VSX_OK) { vsx_plan_destroy(pl); return rc; }
  }
  {
    vsxp::Stopwatch sw(t_run);
    rc = vsx_plan_run(pl);
    if (rc == VSX_OK) rc = vsx_plan_sync(pl, nullptr);
  }
  if (rc == VSX_OK)
    {
      vsxp::Stopwatch sw(t_fetch);
      rc = sink ? fetch_ranked_core(pl, 0, qidx, *sink) : vsx_plan_fetch(pl, out);
    }
  {
    vsxp::Stopwatch sw(t_destroy);
    vsx_plan_destroy(pl);
  }
  if (timing)
    std::fprintf(stderr, "vsx_align_pairs: %llu pairs: plan %.3f s, run+sync %.3f s, fetch %.3f s, destroy %.3f s\n",
                 (unsigned long long) n_pairs, t_plan, t_run, t_fetch, t_destroy);
  return rc;
}

// the slice boundaries of a pipelined call: cut[i] .. cut[i + 1] is slice i (tests/marshal_data.py restates the schedule)
static std::vector<uint64_t> cut_slices(uint64_t n_pairs, uint64_t slice_pairs, const uint32_t * qidx, bool sink /* ranked */)
{
  // slices of about slice_pairs pairs, cut where the query changes (a query's pairs then share tasks as in one plan)
  // (the first and the last slice are half-size: the GPU starts after planning the first one, and the last one's fetch is
  //  the only one nothing overlaps)
  std::vector<uint64_t> cut {0};
  // r04: the slices RAMP -- a quarter and a half slice first, a half and a quarter last.  The timeline of one 800 k-pair call
  // (profiles/r04/r04m_e2e_timeline.txt) is GPU-bound from the first launch to the last kernel, so what the caller waits for beyond
  // the kernels is the planning of the first slice (2.7 ms for 100 k pairs) and the traceback + text + download of the last one;
  // both shrink with their slice, and the planner (15 ns per pair) outruns the GPU (35 ns per pair) by the second slice.
  // Lists shorter than three slices keep the r03 schedule (half, full ..., half).
  std::vector<uint64_t> sizes;
  if (n_pairs >= 3 * slice_pairs)
    {
      const uint64_t head[2] = {slice_pairs / 4, slice_pairs / 2};
      const uint64_t mid = n_pairs - 2 * (head[0] + head[1]);
      const uint64_t k = (mid + slice_pairs - 1) / slice_pairs;
      sizes.push_back(head[0]); sizes.push_back(head[1]);
      for (uint64_t x = 0; x < k; ++x) sizes.push_back(mid * (x + 1) / k - mid * x / k);
      sizes.push_back(head[1]); sizes.push_back(head[0]);
    }
  size_t next_size = 0;
  while (cut.back() < n_pairs)
    {
      const uint64_t left = n_pairs - cut.back();
      uint64_t want = slice_pairs;
      if (!sizes.empty()) want = next_size < sizes.size() ? sizes[next_size++] : left;
      else if (cut.size() == 1) want = slice_pairs / 2;
      else if (left <= slice_pairs / 2 + slice_pairs / 8) want = left;
      else if (left <= slice_pairs + slice_pairs / 2) want = left - slice_pairs / 2;
      uint64_t e = std::min<uint64_t>(n_pairs, cut.back() + want);
      const uint64_t limit = sink ? n_pairs : std::min<uint64_t>(n_pairs, e + want / 2);      // ranked: a query is never split
      while (e < limit && qidx[e] == qidx[e - 1]) ++e;
      if (n_pairs - e < slice_pairs / 16) e = n_pairs;
      cut.push_back(e);
    }
  return cut;
}

// Large pair lists run as a PIPELINE of plans over contiguous slices (cut at query boundaries): a helper thread plans slice
// i+1 (host grouping, task upload) while the GPU runs slice i and the caller's thread fetches slice i-1 (download, CIGAR
// text); the slices' results are concatenated.  Same results as one plan -- a pair's alignment does not depend on its
// batch.  VSX_PIPELINE=0 switches it off.
static int align_pairs_impl(vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                            const uint32_t * qidx, const uint32_t * tidx, const vsx_filter * filter, vsx_results * out, RankedSink * sink)
{
  static const bool pipeline_off = std::getenv("VSX_PIPELINE") && std::strcmp(std::getenv("VSX_PIPELINE"), "0") == 0;
  // slice size: VSX_PIPELINE_SLICE, else a quarter of the list within [128 k, 2 M] pairs -- mid-sized lists (one search
  // stage of 100 k queries = 800 k pairs) overlap planning, kernels and the fetch as well; below 256 k pairs one plan
  static const uint64_t forced_slice = std::getenv("VSX_PIPELINE_SLICE") ? std::max<uint64_t>(64, std::strtoull(std::getenv("VSX_PIPELINE_SLICE"), nullptr, 10)) : 0;
  const uint64_t slice_pairs = forced_slice ? forced_slice : std::min<uint64_t>(2ull << 20, std::max<uint64_t>(128ull << 10, n_pairs / 4));
  if (pipeline_off || !ctx || (!out && !sink) || !queries || !targets || !qidx || !tidx || n_pairs < 2 * slice_pairs)
    return align_pairs_single(ctx, queries, targets, n_pairs, qidx, tidx, filter, out, sink);
  static const bool timing = std::getenv("VSX_DEBUG_TIMING") != nullptr;
  const double t_begin = vsxp::now_s();
  if (out) std::memset(out, 0, sizeof *out);
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(VSX_EHIP, "vsx_align_pairs: hipSetDevice failed");

  const std::vector<uint64_t> cut = cut_slices(n_pairs, slice_pairs, qidx, sink != nullptr);
  const size_t S = cut.size() - 1;
  const uint64_t slice_budget = 0;       // the context's shared checkpoint block (the plans execute in stream order)
  std::vector<vsx_plan *> plans(S, nullptr);
  if (!sink)
    {
      const int arc = results_alloc(out, n_pairs, filter != nullptr);
      if (arc != VSX_OK) return arc;
    }
  std::mutex mu;
  std::condition_variable cv;
  size_t consumed = 0, planned = 0;      // slices [0, planned) have been planned; a failed one is the last and leaves plans[i] null
  bool stop = false;
  int plan_failed = VSX_OK;
  std::string plan_failed_msg;
  const size_t depth = 2;
  // One planner thread, in slice order.  r06 measured two and three (plans of one context may be made concurrently: pool, block and
  // slot choices are locked, uploads share stream_up): a planner needs 2.1-2.8 ms per slice where the GPU needs 5.3, so a second one
  // only adds contention: 29.9 / 31.2 ms per 800 k-pair call with one, 30.6 / 35.4 with two, 30.8 with three
  // (profiles/r06/r06r_e2e_planners_ab.txt).  What the call loses against its 25.4 ms of kernels is on the device: the traceback of
  // slice i runs starved beside the DP kernels of slices i + 1, i + 2 (a retiring DP wave frees 128 VGPRs, a traceback wave needs 168),
  // and the slice that reuses its checkpoint block waits for it.
  std::thread planner([&]() {
    (void) hipSetDevice(ctx->device);
    for (size_t i = 0; i < S; ++i)
      {
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return stop || i < consumed + depth + 2; });      // at most depth + 2 plans alive beyond the fetched ones
          if (stop) return;
        }
        vsx_plan * pl = nullptr;
        int rc = vsx_plan_create(ctx, &pl, queries, targets, cut[i + 1] - cut[i], qidx + cut[i], tidx + cut[i], slice_budget);
        if (rc == VSX_OK && filter) rc = vsx_plan_set_filter(pl, filter);
        if (rc == VSX_OK && sink) rc = plan_set_ranked(pl);
        std::string err;
        if (rc != VSX_OK) { err = vsx_last_error(); if (pl) vsx_plan_destroy(pl); pl = nullptr; }
        if (timing) std::fprintf(stderr, "  slice %zu (%llu pairs): planned at %.1f ms\n", i, (unsigned long long) (cut[i + 1] - cut[i]), (vsxp::now_s() - t_begin) * 1e3);
        std::lock_guard<std::mutex> lk(mu);
        plans[i] = pl; planned = i + 1;
        if (rc != VSX_OK) { plan_failed = rc; plan_failed_msg = err; }
        cv.notify_all();                                           // (also wakes the consumer waiting on a failed plan)
        if (rc != VSX_OK) return;
      }
  });
  int rc = VSX_OK;
  std::string msg;
  size_t launched = 0;
  auto finish = [&](size_t i) {           // fetch slice i straight into its part of the result arrays, release it
    const double tf0 = vsxp::now_s();
    int frc = sink ? fetch_ranked_core(plans[i], cut[i], qidx + cut[i], *sink) : fetch_core(plans[i], dest_at(out, cut[i]));
    if (timing)
      {
        vsx_timing tm;
        if (vsx_plan_sync(plans[i], &tm) == VSX_OK)
          std::fprintf(stderr, "  slice %zu: fetch %.1f .. %.1f ms, kernels %.2f ms (fwd %.2f tb %.2f)\n", i, (tf0 - t_begin) * 1e3, (vsxp::now_s() - t_begin) * 1e3,
                       tm.total_ms, tm.forward_ms, tm.traceback_ms);
      }
    vsx_plan_destroy(plans[i]);
    plans[i] = nullptr;
    { std::lock_guard<std::mutex> lk(mu); consumed = i + 1; }
    cv.notify_all();
    return frc;
  };
  for (size_t i = 0; i < S && rc == VSX_OK; ++i)
    {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return i < planned; });
        if (!plans[i]) { rc = plan_failed; msg = plan_failed_msg; break; }
      }
      // odd slices launch their DP kernels on the second DP stream: a slice is ~3-6 rounds of resident waves, its last round drains
      // for about half a wave's lifetime, and a launch on the same stream would wait for that (inputs are complete: plan_create
      // has synchronised its uploads; the two checkpoint blocks alternate the same way)
      plans[i]->alt_fwd = (i & 1) != 0;
      rc = vsx_plan_run(plans[i]);                       // asynchronous: queued behind slice i-1 on the context's streams
      if (timing) std::fprintf(stderr, "  slice %zu: queued at %.1f ms\n", i, (vsxp::now_s() - t_begin) * 1e3);
      if (rc != VSX_OK) { msg = vsx_last_error(); break; }
      launched = i + 1;
      // `depth` slices stay queued behind the one being fetched: the DP kernels of slice i+1 overlap
      // the traceback of slice i, so the GPU needs the next launch in its queue before the previous slice has drained.  r04 A/B
      // (profiles/r04/r04q_e2e_depth_ab.txt): 3 or 4 queued slices are no better -- a traceback makes little progress beside the DP
      // kernels queued after it (its waves need 256 VGPRs, a retiring DP wave frees 128), so deeper queues only move the wait.
      if (i >= depth) { rc = finish(i - depth); if (rc != VSX_OK) msg = vsx_last_error(); }
    }
  for (size_t i = (launched >= depth ? launched - depth : 0); i < launched && rc == VSX_OK && launched == S; ++i)
    { rc = finish(i); if (rc != VSX_OK) msg = vsx_last_error(); }
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  planner.join();
  for (size_t i = 0; i < S; ++i)
    if (plans[i]) { vsx_plan_destroy(plans[i]); plans[i] = nullptr; }
  if (rc != VSX_OK)
    {
      if (out) vsx_results_free(out);
      vsx_internal_set_error(msg.c_str());
      return rc;
    }
  if (timing)
    std::fprintf(stderr, "vsx_align_pairs: %llu pairs in %zu pipelined slices: %.3f s\n", (unsigned long long) n_pairs, S, vsxp::now_s() - t_begin);
  return VSX_OK;
}

int vsx_align_pairs_filtered(vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                             const uint32_t * qidx, const uint32_t * tidx, const vsx_filter * filter, vsx_results * out)
{
  if (!out) return fail(VSX_EINVAL, "vsx_align_pairs: null argument");
  return align_pairs_impl(ctx, queries, targets, n_pairs, qidx, tidx, filter, out, nullptr);
}

int vsx_align_pairs_ranked(vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                           const uint32_t * qidx, const uint32_t * tidx, const vsx_filter * filter, int keep_weak, vsx_ranked * out)
{
  if (!ctx || !out || !queries || !targets || (n_pairs && (!qidx || !tidx))) return fail(VSX_EINVAL, "vsx_align_pairs_ranked: null argument");
  std::memset(out, 0, sizeof *out);
  if (!filter) return fail(VSX_EINVAL, "vsx_align_pairs_ranked: the ranking needs the accept filter");
  RankedSink sink;
  sink.keep_weak = keep_weak ? 1 : 0;
  const int rc = align_pairs_impl(ctx, queries, targets, n_pairs, qidx, tidx, filter, nullptr, &sink);
  if (rc != VSX_OK) return rc;
  out->n_pairs = n_pairs;
  out->n_hits = sink.pair.size();
  out->pair = dup_array(sink.pair); out->score = dup_array(sink.score); out->aligned = dup_array(sink.aligned);
  out->matches = dup_array(sink.matches); out->mismatches = dup_array(sink.mismatches); out->gaps = dup_array(sink.gaps);
  out->verdict = dup_array(sink.verdict); out->id = dup_array(sink.id); out->cigar_off = dup_array(sink.cigar_off);
  out->n_undecided = sink.undecided.size();
  out->undecided = dup_array(sink.undecided);
  out->cigar_blob = sink.blob ? sink.blob : (char *) std::malloc(1);
  out->cigar_bytes = sink.blob_used;
  sink.blob = nullptr;
  if (!out->pair || !out->score || !out->aligned || !out->matches || !out->mismatches || !out->gaps || !out->verdict || !out->id ||
      !out->cigar_off || !out->undecided || !out->cigar_blob)
    { vsx_ranked_free(out); return fail(VSX_ENOMEM, "vsx_align_pairs_ranked: host allocation failed"); }
  return VSX_OK;
}

}  // extern "C"
