// vsx_allpairs.cpp -- --allpairs_global on the searcher of vsx_search.cpp (vsx_allpairs_rows / _stream / _block, include/vsx_search.h).
//
// allpairs_global (commands/allpairs_global.cpp:394-527): queries [first, first+count) of the database, each
// against every LATER sequence that passes the unaligned filters (or all of them with acceptall); one GPU
// plan for the whole block; hits kept if acceptall or accepted; order allpairs_hit_compare (:116-138).
// allpairs in three stages (r05: vsx_allpairs_stream overlaps them across blocks; vsx_allpairs_rows runs them back to back):
//   A  ap_enumerate  the pair list of a block of rows            host threads
//   B  ap_align      DP + traceback + filter + ranking            the searcher's aligner context (one call at a time)
//   C  ap_complete   derived hit fields, order, marshalling       host threads
#include "vsx_search_internal.h"

using namespace vsxs;

namespace {
struct ApList {
  std::vector<uint32_t> rows;
  std::unique_ptr<uint32_t[]> pq_buf, pt_buf;      // (plain arrays: a vector would zero 2 x 200 MB per block of 1 000 queries before the threads fill them)
  uint64_t n_list = 0;
  std::vector<uint64_t> qfirst, cell_part;
  double t_begin = 0;
};
struct ApAligned {
  bool ranked = false, have_rk = false, have_res = false;
  vsx_ranked rk;
  vsx_results res;
  double t_align = 0;
  ApAligned() { std::memset(&rk, 0, sizeof rk); std::memset(&res, 0, sizeof res); }
  ApAligned(const ApAligned &) = delete;
  ApAligned & operator=(const ApAligned &) = delete;
  ~ApAligned() { if (have_rk) vsx_ranked_free(&rk); if (have_res) vsx_results_free(&res); }
};
}

// stage A: each query of the block against every later sequence that passes the unaligned filters -- per-query target lists on host
// threads, concatenated in query order
static int ap_enumerate(const vsx_searcher * S, int32_t acceptall, const uint32_t * rows_in, uint64_t count, ApList & L, int thread_budget)
{
  const uint64_t n = S->len.size();
  L.t_begin = now_s();
  L.rows.assign(rows_in, rows_in + count);
  const uint32_t * rows = L.rows.data();
  std::unique_ptr<uint32_t[]> & pq_buf = L.pq_buf, & pt_buf = L.pt_buf;
  uint32_t * pq = nullptr, * pt = nullptr;
  uint64_t & n_list = L.n_list;
  std::vector<uint64_t> & qfirst = L.qfirst, & cell_part = L.cell_part;
  qfirst.assign(count + 1, 0);
  {
    std::vector<std::vector<uint32_t>> tl(count);
    const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, thread_budget), count / 8));
    std::atomic<uint64_t> next {0};
    // search_acceptable_unaligned (searchcore.cpp:541-609) is true for EVERY pair when all twelve of its options sit at their defaults and
    // no sequence carries an abundance annotation (abundance 1 everywhere: the ratio clauses compare 1 with 0 and with DBL_MAX)
    const vsx_search_opts & fo = S->o;
    const bool inert = fo.maxqsize == INT64_MAX && fo.mintsize <= 1 && fo.minsizeratio == 0.0 && fo.maxsizeratio == DBL_MAX && fo.minqt == 0.0 &&
                       fo.maxqt == DBL_MAX && fo.minsl == 0.0 && fo.maxsl == DBL_MAX && fo.idprefix == 0 && fo.idsuffix == 0 && fo.self == 0 &&
                       fo.selfid == 0 && S->tsize.empty();
    auto work = [&]() {
      for (;;)
        {
          const uint64_t k = next.fetch_add(1);
          if (k >= count) break;
          const uint64_t qi = rows[k];
          std::vector<uint32_t> & v = tl[k];
          if (acceptall || inert)
            {
              // every later sequence: no filter to ask (r05: the 1.25e9 predicate calls of a 50 000-sequence run were most of the
              // ~3 s of pair enumeration that no align call overlapped)
              v.resize(n - qi - 1);
              for (uint64_t t = qi + 1; t < n; ++t) v[t - qi - 1] = (uint32_t) t;
              continue;
            }
          v.reserve(n - qi);
          for (uint64_t t = qi + 1; t < n; ++t)
            if (acceptable_unaligned(*S, S->blob.data() + S->off[qi], S->len[qi], (uint32_t) t, S->meta_of(qi))) v.push_back((uint32_t) t);
        }
    };
    run_pool(nth, [&](int) { work(); });
    uint64_t total = 0;
    for (uint64_t k = 0; k < count; ++k) { qfirst[k] = total; total += tl[k].size(); }
    qfirst[count] = total;
    pq_buf.reset(new uint32_t[std::max<uint64_t>(total, 1)]); pt_buf.reset(new uint32_t[std::max<uint64_t>(total, 1)]);
    pq = pq_buf.get(); pt = pt_buf.get(); n_list = total;
    // the concatenation and the cell count on the same threads (r04: as serial loops over 5e7 pairs they were ~0.1 s of a 0.8 s block
    // of 1 000 queries at 50 000 sequences)
    cell_part.assign(count, 0);
    std::atomic<uint64_t> next2 {0};
    auto place = [&]() {
      for (;;)
        {
          const uint64_t k = next2.fetch_add(1);
          if (k >= count) break;
          std::fill(pq + qfirst[k], pq + qfirst[k + 1], rows[k]);
          std::copy(tl[k].begin(), tl[k].end(), pt + qfirst[k]);
          uint64_t tlen = 0;
          for (uint32_t t : tl[k]) tlen += S->len[t];
          cell_part[k] = (uint64_t) S->len[rows[k]] * tlen;
          std::vector<uint32_t>().swap(tl[k]);
        }
    };
    std::vector<std::thread> pool2;
    for (int t = 1; t < nth; ++t) pool2.emplace_back(place);
    place();
    for (auto & th : pool2) th.join();
  }
  return VSX_OK;
}

// the device decides (and ranks) unless every pair's record is wanted (acceptall) or the host filters (gap_infinite, unoise)
static bool ap_ranked(const vsx_searcher * S, int32_t acceptall) { return !(acceptall || S->o.gap_infinite || S->o.cluster_unoise); }

// stage B: the block's pairs through the aligner.  Ranked path (vsx_rank.hip): the device filters, orders (id desc, target asc per
// query: allpairs_hit_compare :116-138) and compacts; only accepted pairs come back.  Otherwise every pair's record, with the verdicts.
static int ap_align(vsx_searcher * S, int32_t acceptall, const ApList & L, ApAligned & A)
{
  const double t0 = now_s();
  const vsx_filter flt = make_filter(*S);
  A.ranked = ap_ranked(S, acceptall);
  int rc;
  if (A.ranked)
    {
      rc = vsx_align_pairs_ranked(S->ctx, S->dbset, S->dbset, L.n_list, L.pq_buf.get(), L.pt_buf.get(), &flt, 0, &A.rk);
      A.have_rk = rc == VSX_OK;
    }
  else
    {
      rc = vsx_align_pairs_filtered(S->ctx, S->dbset, S->dbset, L.n_list, L.pq_buf.get(), L.pt_buf.get(), nullptr, &A.res);
      A.have_res = rc == VSX_OK;
    }
  A.t_align = now_s() - t0;
  return rc;
}

// allpairs_hit_compare (commands/allpairs_global.cpp:116-138): id descending, target ascending
static bool allpairs_hit_less(const Hit & a, const Hit & b)
{
  if (a.id != b.id) return a.id > b.id;
  return a.target < b.target;
}

static int complete_error(int code)
{
  return fail(code, code == VSX_EHIP ? "vsx_allpairs_rows: device and host accept filters disagree" : "vsx_allpairs_rows: fallback aligner failed");
}

// stage C, ranked: the device has filtered, ordered and compacted; the host completes the derived fields of what came back
static int complete_ranked(vsx_searcher * S, const ApList & L, ApAligned & A, std::vector<std::vector<Hit>> & kept, uint64_t & sentinels, int thread_budget)
{
  const uint64_t count = L.rows.size();
  const uint32_t * rows = L.rows.data();
  const uint32_t * pt = L.pt_buf.get();
  const std::vector<uint64_t> & qfirst = L.qfirst;
  vsx_ranked & rk = A.rk;
  vsx_results view;
  std::memset(&view, 0, sizeof view);
  view.n_pairs = rk.n_hits; view.score = rk.score; view.aligned = rk.aligned; view.matches = rk.matches;
  view.mismatches = rk.mismatches; view.gaps = rk.gaps; view.cigar_off = rk.cigar_off; view.cigar_blob = rk.cigar_blob;
  // hits are grouped by query in list order: group boundaries by one sweep
  std::vector<uint64_t> hfirst(count + 1, 0);
  {
    uint64_t j = 0;
    for (uint64_t k = 0; k < count; ++k)
      {
        hfirst[k] = j;
        while (j < rk.n_hits && rk.pair[j] < qfirst[k + 1]) ++j;      // (inside a group the pair indices follow the ranking)
      }
    hfirst[count] = j;
  }
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, thread_budget), count / 8));
  std::vector<int> err((size_t) nth, VSX_OK);
  std::atomic<uint64_t> next {0}, rank_drift {0};
  static const bool rank_strict = std::getenv("VSX_RANK_STRICT") != nullptr;
  auto work = [&](int tid) {
    uint64_t dummy = 0;
    for (;;)
      {
        const uint64_t k = next.fetch_add(1);
        if (k >= count) break;
        const uint64_t qi = rows[k];
        const char * q = S->blob.data() + S->off[qi];
        const int64_t ql = S->len[qi];
        kept[k].reserve(hfirst[k + 1] - hfirst[k]);
        bool resort = false;
        for (uint64_t j = hfirst[k]; j < hfirst[k + 1]; ++j)
          {
            Hit h;
            h.target = pt[rk.pair[j]];
            const int frc = fill_hit(*S, [&]() { return q; }, ql, h, view, j, dummy);
            if (frc != VSX_OK) { err[(size_t) tid] = frc; return; }
            // The device's filter and identity are the same double expressions as the host's (vsx_rank.hip) and the soaks compare
            // them bit for bit (VSX_RANK_STRICT=1 turns any difference into an error there).  In production a difference -- a host
            // build with other floating-point flags, say -- must not fail the run: the host value stands, the group is re-ordered
            // by it, a hit the host would not accept is dropped, and the count is reported once.
            const bool ok = acceptable_aligned(*S, ql, h, S->abundance(qi));
            if (!ok || h.id != rk.id[j])
              {
                if (rank_strict) { err[(size_t) tid] = VSX_EHIP; return; }
                rank_drift.fetch_add(1);
                resort = true;
                if (!ok) continue;
              }
            kept[k].push_back(std::move(h));
          }
        if (resort) std::stable_sort(kept[k].begin(), kept[k].end(), allpairs_hit_less);
      }
  };
  run_pool(nth, work);
  for (int t = 0; t < nth; ++t)
    if (err[(size_t) t] != VSX_OK) return complete_error(err[(size_t) t]);
  if (rank_drift.load())
    {
      static std::atomic<bool> told {false};
      if (!told.exchange(true))
        std::fprintf(stderr, "vsx_allpairs_rows: %llu hit(s) where the device's identity or filter differs from the host's; the host values stand\n",
                     (unsigned long long) rank_drift.load());
    }
  // pairs the 16-bit aligner refused: linear-memory fallback, host filter, ordered insertion (rare)
  for (uint64_t u = 0; u < rk.n_undecided; ++u)
    {
      const uint64_t r = rk.undecided[u];
      const uint64_t k = (uint64_t) (std::upper_bound(qfirst.begin(), qfirst.end(), r) - qfirst.begin()) - 1;
      const uint64_t qi = rows[k];
      int16_t sc = VSX_SCORE_SENTINEL; uint16_t z = 0; uint64_t zo = 0; char e0 = 0;
      vsx_results one;
      std::memset(&one, 0, sizeof one);
      one.n_pairs = 1; one.score = &sc; one.aligned = &z; one.matches = &z; one.mismatches = &z; one.gaps = &z; one.cigar_off = &zo; one.cigar_blob = &e0;
      Hit h;
      h.target = pt[r];
      const char * q = S->blob.data() + S->off[qi];
      const int frc = fill_hit(*S, [&]() { return q; }, (int64_t) S->len[qi], h, one, 0, sentinels);
      if (frc != VSX_OK) return fail(frc, "vsx_allpairs_rows: fallback aligner failed");
      if (acceptable_aligned(*S, S->len[qi], h, S->abundance(qi)))
        {
          kept[k].push_back(std::move(h));
          std::stable_sort(kept[k].begin(), kept[k].end(), allpairs_hit_less);
        }
    }
  return VSX_OK;
}

// stage C, every pair's record: per query, complete the accepted hits (derived fields, fallback on the sentinel) and order them
static int complete_unranked(vsx_searcher * S, int32_t acceptall, const ApList & L, ApAligned & A, std::vector<std::vector<Hit>> & kept, uint64_t & sentinels,
                             int thread_budget)
{
  const uint64_t count = L.rows.size();
  const uint32_t * rows = L.rows.data();
  const uint32_t * pt = L.pt_buf.get();
  const std::vector<uint64_t> & qfirst = L.qfirst;
  vsx_results & res = A.res;
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, thread_budget), count / 8));
  std::vector<uint64_t> psent((size_t) nth, 0);
  std::vector<int> err((size_t) nth, VSX_OK);
  std::atomic<uint64_t> next {0};
  auto work = [&](int tid) {
    for (;;)
      {
        const uint64_t k = next.fetch_add(1);
        if (k >= count) break;
        const uint64_t qi = rows[k];
        const char * q = S->blob.data() + S->off[qi];
        const int64_t ql = S->len[qi];
        for (uint64_t r = qfirst[k]; r < qfirst[k + 1]; ++r)
          {
            Hit h;
            h.target = pt[r];
            const uint8_t verdict = res.verdict ? res.verdict[r] : (uint8_t) VSX_VERDICT_UNDECIDED;
            if (verdict == VSX_VERDICT_REJECTED || verdict == VSX_VERDICT_WEAK) continue;      // only accepted hits are kept (:509-527)
            const int frc = fill_hit(*S, [&]() { return q; }, ql, h, res, r, psent[(size_t) tid]);
            if (frc != VSX_OK) { err[(size_t) tid] = frc; return; }
            const bool acc = acceptall || acceptable_aligned(*S, ql, h, S->abundance(qi));
            if (verdict == VSX_VERDICT_ACCEPTED && !acc) { err[(size_t) tid] = VSX_EHIP; return; }
            if (acc) kept[k].push_back(std::move(h));
          }
        std::sort(kept[k].begin(), kept[k].end(), allpairs_hit_less);
      }
  };
  run_pool(nth, work);
  for (int t = 0; t < nth; ++t)
    {
      sentinels += psent[(size_t) t];
      if (err[(size_t) t] != VSX_OK) return complete_error(err[(size_t) t]);
    }
  return VSX_OK;
}

// stage C: the host completes the derived fields of the kept hits, orders them and marshals the block's result
static int ap_complete(vsx_searcher * S, int32_t acceptall, const ApList & L, ApAligned & A, vsx_hits * out, int thread_budget)
{
  const uint64_t count = L.rows.size();
  const uint32_t * rows = L.rows.data();
  std::memset(out, 0, sizeof *out);
  std::vector<std::vector<Hit>> kept(count);
  uint64_t cells = 0, sentinels = 0;
  for (uint64_t k = 0; k < count; ++k) cells += L.cell_part[k];
  int rc = A.ranked ? complete_ranked(S, L, A, kept, sentinels, thread_budget) : complete_unranked(S, acceptall, L, A, kept, sentinels, thread_budget);
  if (rc != VSX_OK) return rc;
  rc = marshal_hits(kept, out, thread_budget);
  if (rc != VSX_OK) return rc;
  for (uint64_t k = 0; k < out->n_hits; ++k) out->hit[k].query = rows[out->hit[k].query];       // vsx_hit.query = database sequence number
  out->pairs_aligned = L.n_list; out->cells_aligned = cells; out->stages = 1; out->sentinel_pairs = sentinels;
  out->seconds_align = A.t_align; out->seconds_total = now_s() - L.t_begin;
  return VSX_OK;
}

extern "C" {

int vsx_allpairs_rows(vsx_searcher * S, int32_t acceptall, const uint32_t * rows, uint64_t count, vsx_hits * out)
{
  if (!S || !out || (count && !rows)) return fail(VSX_EINVAL, "vsx_allpairs_rows: null argument");
  std::memset(out, 0, sizeof *out);
  const uint64_t n = S->len.size();
  for (uint64_t k = 0; k < count; ++k)
    if (rows[k] >= n || (k && rows[k] <= rows[k - 1])) return fail(VSX_EINVAL, "vsx_allpairs_rows: rows must be ascending database sequence numbers");
  ApList L;
  int rc = ap_enumerate(S, acceptall, rows, count, L, S->threads);
  if (rc != VSX_OK) return rc;
  ApAligned A;
  rc = ap_align(S, acceptall, L, A);
  if (rc != VSX_OK) return rc;
  return ap_complete(S, acceptall, L, A, out, S->threads);
}

// allpairs_global as ONE call (commands/allpairs_global.cpp:394-527 runs its query loop on worker threads and reports each query as it
// finishes): the rows first .. first + count - 1 in blocks of `block` queries, the three stages of consecutive blocks overlapped -- while
// block i is on the GPU, block i + 1's pair list is enumerated and block i - 1's hits are completed on host threads (r04: 4.0 of the
// 53.4 s of a 50 000-sequence run lay outside the align calls and overlapped nothing).  `sink` receives every block's hits, in order,
// on a helper thread (one call at a time); the hits belong to the library and die when the sink returns.  A non-zero return of the
// sink stops the run and is handed back.
int vsx_allpairs_stream(vsx_searcher * S, int32_t acceptall, uint64_t first, uint64_t count, uint64_t block, vsx_hits_sink sink, void * user)
{
  if (!S || !sink) return fail(VSX_EINVAL, "vsx_allpairs_stream: null argument");
  const uint64_t n = S->len.size();
  if (first > n || count > n - first) return fail(VSX_EINVAL, "vsx_allpairs_stream: query block out of range");
  if (block == 0) block = 1000;
  const uint64_t nb = (count + block - 1) / block;
  const int side = std::max(1, S->threads / 2);                  // enumeration and completion run beside each other and beside the planner of stage B
  auto rows_of = [&](uint64_t b) {
    const uint64_t lo = first + b * block, hi = std::min(first + count, lo + block);
    std::vector<uint32_t> r(hi - lo);
    for (uint64_t k = 0; k < hi - lo; ++k) r[k] = (uint32_t) (lo + k);
    return r;
  };
  struct Done { int rc = VSX_OK; std::string msg; };
  // block 0's list AND block 1's before the first align call: the first call of a process allocates its checkpoint blocks (tens of GB of
  // hipMalloc, 0.9 - 7 s from box to box: profiles/r05/r05f_allpairs_stream_first_build.txt, r05g_allpairs_20k_stream_ab.txt), and nothing
  // should compete with it for the kernel's memory-management locks.  From block 1 on the next list is built beside the GPU.
  std::unique_ptr<ApList> next(new ApList), ahead;
  if (nb)
    {
      const std::vector<uint32_t> r = rows_of(0);
      const int rc0 = ap_enumerate(S, acceptall, r.data(), r.size(), *next, S->threads);
      if (rc0 != VSX_OK) return rc0;
    }
  if (nb > 1)
    {
      ahead.reset(new ApList);
      const std::vector<uint32_t> r = rows_of(1);
      const int rc1 = ap_enumerate(S, acceptall, r.data(), r.size(), *ahead, S->threads);
      if (rc1 != VSX_OK) return rc1;
    }
  std::thread enum_thread, done_thread;
  Done enum_done, comp_done;
  auto join = [](std::thread & t) { if (t.joinable()) t.join(); };
  int rc = VSX_OK;
  std::string msg;
  for (uint64_t b = 0; b < nb && rc == VSX_OK; ++b)
    {
      std::unique_ptr<ApList> cur = std::move(next);
      if (b == 0 && ahead) next = std::move(ahead);              // (built before the loop)
      else next.reset(new ApList);
      if (b + 1 < nb && b >= 1)
        {
          ApList * dst = next.get();
          enum_done = Done {};
          enum_thread = std::thread([&, dst, b]() {
            const std::vector<uint32_t> r = rows_of(b + 1);
            enum_done.rc = ap_enumerate(S, acceptall, r.data(), r.size(), *dst, side);
            if (enum_done.rc != VSX_OK) enum_done.msg = vsx_last_error();
          });
        }
      std::unique_ptr<ApAligned> A(new ApAligned);
      rc = ap_align(S, acceptall, *cur, *A);
      if (rc != VSX_OK) msg = vsx_last_error();
      join(done_thread);                                         // block b - 1 has been handed to the sink
      if (rc == VSX_OK && comp_done.rc != VSX_OK) { rc = comp_done.rc; msg = comp_done.msg; }
      if (rc == VSX_OK)
        {
          ApList * lp = cur.release();
          ApAligned * ap = A.release();
          const uint64_t bfirst = first + b * block;
          comp_done = Done {};
          done_thread = std::thread([&, lp, ap, bfirst]() {
            std::unique_ptr<ApList> lo(lp);
            std::unique_ptr<ApAligned> ao(ap);
            vsx_hits h;
            int crc = ap_complete(S, acceptall, *lo, *ao, &h, side);
            if (crc != VSX_OK) { comp_done.rc = crc; comp_done.msg = vsx_last_error(); return; }
            ao.reset();                                          // (the device-side results are copied: free them before the sink runs)
            const int src = sink(user, bfirst, lo->rows.size(), &h);
            vsx_hits_free(&h);
            if (src != 0) { comp_done.rc = src; comp_done.msg = "vsx_allpairs_stream: stopped by the sink"; }
          });
        }
      join(enum_thread);
      if (rc == VSX_OK && b + 1 < nb && b >= 1 && enum_done.rc != VSX_OK) { rc = enum_done.rc; msg = enum_done.msg; }
    }
  join(enum_thread);
  join(done_thread);
  if (rc == VSX_OK && comp_done.rc != VSX_OK) { rc = comp_done.rc; msg = comp_done.msg; }
  if (rc != VSX_OK) vsx_internal_set_error(msg.c_str());
  return rc;
}

int vsx_allpairs_block(vsx_searcher * S, int32_t acceptall, uint64_t first, uint64_t count, vsx_hits * out)
{
  if (!S || !out) return fail(VSX_EINVAL, "vsx_allpairs_block: null argument");
  std::memset(out, 0, sizeof *out);
  const uint64_t n = S->len.size();
  if (first > n || count > n - first) return fail(VSX_EINVAL, "vsx_allpairs_block: query block out of range");
  std::vector<uint32_t> rows(count);
  for (uint64_t k = 0; k < count; ++k) rows[k] = (uint32_t) (first + k);
  return vsx_allpairs_rows(S, acceptall, rows.data(), count, out);
}

}  // extern "C"
