// vsx_exact.cpp -- exact sequence search (include/vsx_search.h: vsx_search_exact), the host side of vsx_exact.hip.
//
// Restated from the reference (src/, v2.31.0):
//   search_exact_onequery / search_exact_query   commands/search_exact.cpp   both strands, every match evaluated, hits joined
//   dbhash_open / dbhash_add / dbhash_search_*   core/dbhash.cpp             hash of the normalised sequence, linear probing,
//                                                                            seqcmp on equal hashes
//   string_normalize                             utils/string_normalize.cpp  the 4-bit codes (chrmap_4bit)
//   search_acceptable_unaligned / _aligned       core/searchcore.cpp:541-609, :664-737
//   search_joinhits                              core/searchcore.cpp:1028-1052
//
// A call runs its queries in windows.  A window is staged in pinned memory (every sequence in a 16-byte aligned slot; with
// --hardmask on the queries both strands are staged as masked text, otherwise the minus strand is read backwards from the plus
// strand's text on the device), hashed and probed on the device, and finished on host threads: each query's matches are sorted
// by (target, strand), filtered and turned into the fixed hit record.  The host restatement replaces only the device part: it
// fills the same per-strand match lists from a std::unordered_multimap over the code strings.
#include "vsx_search_internal.h"
#include "vsx_exact_internal.h"

#include <unordered_map>

using namespace vsxs;
using vsxp::DevBuf;
using vsxp::PinnedBuf;
using vsxp::ensure_pinned;
using vsxp::map4;
using vsxe::Plan;
using vsxe::plan_items;
using vsxe::slot_of;
using vsxe::words_of;
using vsxe::table_size_for;

#define WHO "vsx_search_exact"

struct VsxExactIndex {
  // ---- device: the table, the database's code words and where each sequence's words begin
  bool device_ready = false;
  uint64_t table_size = 0, hash_mask = ~0ull;
  DevBuf<VsxExactSlot> table;
  DevBuf<uint64_t> dbwords, dbwoff;
  // ---- the window's buffers (grow-only, kept between calls)
  PinnedBuf<char> h_text;
  PinnedBuf<VsxExactItem> h_items;
  PinnedBuf<uint32_t> h_cnt, h_hits;
  PinnedBuf<uint64_t> h_start;
  PinnedBuf<VsxExactCounters> h_counters;
  DevBuf<uint8_t> d_text;
  DevBuf<VsxExactItem> d_items;
  DevBuf<uint64_t> d_qwords, d_qhash, d_start;
  DevBuf<uint32_t> d_cnt, d_hits;
  DevBuf<VsxExactCounters> d_counters;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // ---- the host restatement: code string -> database sequence number
  bool host_ready = false;
  std::unordered_multimap<std::string, uint32_t> map;
};

namespace {

thread_local vsx_exact_stats g_stats;

// the window's text: the plus strands copied, the minus strands (own_minus) reverse-complemented from the UNMASKED query and
// every strand masked on its own (core/search.cpp:294-303)
template <typename FSeq>
void fill_text(const vsx_searcher * S, const Plan & P, const VsxExactItem * items, FSeq seq, char * text, bool mask)
{
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S->threads), P.n / 4096 + 1));
  std::atomic<uint64_t> next {0};
  run_pool(nth, [&](int) {
    for (;;)
      {
        const uint64_t k0 = next.fetch_add(1024);
        if (k0 >= P.n) break;
        for (uint64_t k = k0; k < std::min(P.n, k0 + 1024); ++k)
          {
            const char * q = seq(k);
            const uint32_t L = items[k].len;
            if (L) std::memcpy(text + items[k].off, q, L);
            if (P.both && P.own_minus)
              {
                char * d = text + items[P.n + k].off;
                for (uint32_t x = 0; x < L; ++x) d[x] = complement((unsigned char) q[L - 1 - x]);
              }
          }
      }
  });
  if (!mask) return;
  const uint64_t nm = P.own_minus ? P.ns : P.n;
  auto off = [&](uint64_t k) { return items[k].off; };
  auto len = [&](uint64_t k) { return (int64_t) items[k].len; };
  if (S->qmode == 2) dust_states(S, text, nm, off, len, true);
  else hardmask_states(S, text, nm, off, len);
}

// the per-strand match lists of a window, as the probe kernel leaves them
struct Matches { const uint32_t * cnt; const uint64_t * start; const uint32_t * hits; };

// the code string of an item (the host restatement's key)
void codes_of(const VsxExactItem & it, const char * text, std::string & out)
{
  out.resize(it.len);
  const char * p = text + it.off;
  if (!it.reverse) for (uint32_t i = 0; i < it.len; ++i) out[i] = (char) map4((unsigned char) p[i]);
  else for (uint32_t i = 0; i < it.len; ++i) out[i] = (char) map4((unsigned char) complement((unsigned char) p[it.len - 1 - i]));
}

void build_host_index(const vsx_searcher * S, VsxExactIndex & X)
{
  if (X.host_ready) return;
  const double t0 = now_s();
  const uint64_t n = S->len.size();
  X.map.reserve(n);
  std::string key;
  for (uint64_t i = 0; i < n; ++i)
    {
      if (S->len[i] == 0) continue;
      codes_of(VsxExactItem {S->off[i], 0, S->len[i], 0u}, S->blob.data(), key);
      X.map.emplace(key, (uint32_t) i);
    }
  X.host_ready = true;
  g_stats.seconds_index += now_s() - t0;
}

int build_device_index(vsx_searcher * S, VsxExactIndex & X)
{
  if (X.device_ready) return VSX_OK;
  const double t0 = now_s();
  const uint64_t n = S->len.size();
  if (n >= (uint64_t) VSX_EXACT_EMPTY) return fail(VSX_EINVAL, "%s: too many database sequences", WHO);
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
  hipStream_t st = vsx_internal_stream(S->ctx);
  VSX_HIP_AS(WHO, hipEventCreate(&X.ev_a));
  VSX_HIP_AS(WHO, hipEventCreate(&X.ev_b));
  X.hash_mask = vsxe::hash_mask_from_env("VSX_EXACT_HASH_BITS");
  X.table_size = table_size_for(n);
  VSX_HIP_AS(WHO, X.table.alloc(X.table_size));
  VSX_HIP_AS(WHO, hipMemsetAsync(X.table.p, 0xFF, X.table_size * sizeof(VsxExactSlot), st));
  std::vector<uint64_t> woff(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) woff[i + 1] = woff[i] + words_of(S->len[i]);
  VSX_HIP_AS(WHO, X.dbwords.alloc(woff[n] + 2));
  VSX_HIP_AS(WHO, X.dbwoff.alloc(n + 1));
  VSX_HIP_AS(WHO, hipMemcpyAsync(X.dbwoff.p, woff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  DevBuf<uint64_t> d_hash;
  DevBuf<uint32_t> d_len;
  VSX_HIP_AS(WHO, d_hash.alloc(n));
  VSX_HIP_AS(WHO, d_len.alloc(n));
  VSX_HIP_AS(WHO, hipMemcpyAsync(d_len.p, S->len.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  // the database goes through the queries' staging and hash kernel, a block of sequences at a time
  const uint64_t block = 1u << 18;
  for (uint64_t b0 = 0; b0 < n; b0 += block)
    {
      const uint64_t bn = std::min(block, n - b0);
      VSX_HIP_AS(WHO, ensure_pinned(X.h_items, bn));
      const Plan P = plan_items(bn, [&](uint64_t k) { return S->len[b0 + k]; }, false, false, X.h_items.p);
      for (uint64_t k = 0; k < bn; ++k) X.h_items.p[k].woff = woff[b0 + k];
      VSX_HIP_AS(WHO, ensure_pinned(X.h_text, P.text_bytes));
      fill_text(S, P, X.h_items.p, [&](uint64_t k) { return S->blob.data() + S->off[b0 + k]; }, X.h_text.p, false);
      VSX_HIP_AS(WHO, X.d_text.ensure(P.text_bytes));
      VSX_HIP_AS(WHO, X.d_items.ensure(bn));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_text.p, X.h_text.p, P.text_bytes, hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_items.p, X.h_items.p, bn * sizeof(VsxExactItem), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, vsx_launch_exact_hash(X.d_items.p, (uint32_t) bn, X.d_text.p, X.hash_mask, X.dbwords.p, d_hash.p + b0, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));               // the pinned block is staged again
    }
  VSX_HIP_AS(WHO, vsx_launch_exact_insert(d_hash.p, d_len.p, 0, (uint32_t) n, X.table.p, X.table_size, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  X.device_ready = true;
  g_stats.seconds_index += now_s() - t0;
  return VSX_OK;
}

// one window on the device: stage, hash, probe (again with a larger buffer when the hits did not fit), fetch
int device_window(vsx_searcher * S, VsxExactIndex & X, const Plan & P, Matches & M)
{
  hipStream_t st = vsx_internal_stream(S->ctx);
  const uint64_t ns = P.ns;
  VSX_HIP_AS(WHO, X.d_text.ensure(P.text_bytes));
  VSX_HIP_AS(WHO, X.d_items.ensure(ns));
  VSX_HIP_AS(WHO, X.d_qwords.ensure(P.words + 2));
  VSX_HIP_AS(WHO, X.d_qhash.ensure(ns));
  VSX_HIP_AS(WHO, X.d_cnt.ensure(ns));
  VSX_HIP_AS(WHO, X.d_start.ensure(ns));
  VSX_HIP_AS(WHO, X.d_counters.ensure(1));
  VSX_HIP_AS(WHO, X.d_hits.ensure(std::max<uint64_t>(ns, 65536)));
  VSX_HIP_AS(WHO, ensure_pinned(X.h_cnt, ns));
  VSX_HIP_AS(WHO, ensure_pinned(X.h_start, ns));
  VSX_HIP_AS(WHO, ensure_pinned(X.h_counters, 1));
  VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_text.p, X.h_text.p, P.text_bytes, hipMemcpyHostToDevice, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_items.p, X.h_items.p, ns * sizeof(VsxExactItem), hipMemcpyHostToDevice, st));
  VSX_HIP_AS(WHO, hipEventRecord(X.ev_a, st));
  VSX_HIP_AS(WHO, vsx_launch_exact_hash(X.d_items.p, (uint32_t) ns, X.d_text.p, X.hash_mask, X.d_qwords.p, X.d_qhash.p, st));
  for (int attempt = 0; ; ++attempt)
    {
      const uint64_t cap = X.d_hits.n;
      VSX_HIP_AS(WHO, hipMemsetAsync(X.d_counters.p, 0, sizeof(VsxExactCounters), st));
      VSX_HIP_AS(WHO, vsx_launch_exact_probe(X.d_items.p, (uint32_t) ns, X.d_qwords.p, X.d_qhash.p, X.table.p, X.table_size, X.dbwords.p,
                                             X.dbwoff.p, X.d_cnt.p, X.d_start.p, X.d_hits.p, cap, X.d_counters.p, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev_b, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_counters.p, X.d_counters.p, sizeof(VsxExactCounters), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      if (X.h_counters.p->hits <= cap) break;
      if (attempt > 0) return fail(VSX_EHIP, "%s: the probe kernel asked for more hits than it counted", WHO);
      VSX_HIP_AS(WHO, X.d_hits.alloc(X.h_counters.p->hits));    // the exact number: the second launch finds the same matches
    }
  float ms = 0.f;
  VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, X.ev_a, X.ev_b));
  g_stats.seconds_kernel += ms * 1e-3;
  const uint64_t total = X.h_counters.p->hits;
  VSX_HIP_AS(WHO, ensure_pinned(X.h_hits, total));
  VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_cnt.p, X.d_cnt.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_start.p, X.d_start.p, ns * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (total) VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_hits.p, X.d_hits.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.slots_visited += X.h_counters.p->slots_visited;
  g_stats.candidates_compared += X.h_counters.p->candidates_compared;
  M = Matches {X.h_cnt.p, X.h_start.p, X.h_hits.p};
  return VSX_OK;
}

// the same lists from the host map
struct HostLists { std::vector<uint32_t> cnt, hits; std::vector<uint64_t> start; };
void host_window(const VsxExactIndex & X, const Plan & P, const VsxExactItem * items, const char * text, HostLists & L, Matches & M)
{
  L.cnt.assign(P.ns, 0); L.start.assign(P.ns, 0); L.hits.clear();
  std::string key;
  for (uint64_t k = 0; k < P.ns; ++k)
    {
      if (items[k].len == 0) continue;
      codes_of(items[k], text, key);
      const auto range = X.map.equal_range(key);
      L.start[k] = L.hits.size();
      for (auto it = range.first; it != range.second; ++it) { L.hits.push_back(it->second); ++g_stats.candidates_compared; }
      L.cnt[k] = (uint32_t) (L.hits.size() - L.start[k]);
    }
  M = Matches {L.cnt.data(), L.start.data(), L.hits.data()};
}

// a block of consecutive queries finished on one thread
struct Block { std::vector<Hit> hits; std::vector<uint32_t> per_query; };

// search_exact_onequery's evaluation of the matches of queries [b, e) of a window
void finish_queries(const vsx_searcher & S, const Plan & P, const Matches & M, uint64_t b, uint64_t e, uint64_t w0, const uint32_t * qlen,
                    const vsx_seq_meta * qmeta, Block & out)
{
  std::vector<uint64_t> found;                        // (target << 1) | strand
  out.per_query.assign(e - b, 0);
  for (uint64_t k = b; k < e; ++k)
    {
      found.clear();
      for (int strand = 0; strand < (P.both ? 2 : 1); ++strand)
        {
          const uint64_t item = k + (uint64_t) strand * P.n;
          for (uint32_t x = 0; x < M.cnt[item]; ++x) found.push_back(((uint64_t) M.hits[M.start[item] + x] << 1) | (uint64_t) strand);
        }
      if (found.empty()) continue;
      std::sort(found.begin(), found.end());
      const uint64_t qi = w0 + k;
      const int64_t ql = qlen[qi];
      const QMeta qm {(qmeta && qmeta->abundance) ? (int64_t) qmeta->abundance[qi] : 1, (qmeta && qmeta->label) ? qmeta->label[qi] : nullptr};
      for (const uint64_t f : found)
        {
          const uint32_t target = (uint32_t) (f >> 1);
          // the symbol-comparing filters (idprefix, idsuffix, selfid) read the strand that matched: code for code the target itself
          if (!acceptable_unaligned(S, S.blob.data() + S.off[target], ql, target, qm)) continue;
          Hit h;
          h.target = target; h.minus = (f & 1) != 0; h.aligned = true;
          h.nwscore = (int) (ql * S.scoring.match);
          h.nwalignmentlength = h.matches = h.internal_alignmentlength = h.shortest = h.longest = (int) ql;
          h.nwid = h.id = h.id0 = h.id1 = h.id2 = h.id3 = h.id4 = 100.0;
          h.cigar = std::to_string(ql) + "M";
          if (!acceptable_aligned(S, ql, h, qm.qsize)) continue;
          out.hits.push_back(std::move(h));
          ++out.per_query[k - b];
        }
    }
}

int run(vsx_searcher * S, bool host_all, uint64_t nq, const char * qblob, const uint64_t * qoff, const uint32_t * qlen,
        const vsx_seq_meta * qmeta, vsx_hits * out)
{
  if (!S->xidx) S->xidx = new VsxExactIndex;
  VsxExactIndex & X = *S->xidx;
  if (host_all) build_host_index(S, X);
  else { const int rc = build_device_index(S, X); if (rc != VSX_OK) return rc; }

  const bool both = S->o.strand_both != 0;
  // masking the queries changes a match only when the masked symbols become 'N' (--hardmask on the queries, any mode but none)
  const bool hardq = (S->o.hardmask & 2) != 0 && S->qmode != 0;
  const uint64_t window = S->o.window > 0 ? (uint64_t) S->o.window : 65536;
  std::vector<std::unique_ptr<Block>> blocks;
  std::vector<HitSpan> span(nq, HitSpan {nullptr, 0});
  std::vector<char> host_text;
  std::vector<VsxExactItem> host_items;
  HostLists lists;
  const uint64_t per_block = 2048;

  for (uint64_t w0 = 0; w0 < nq; w0 += window)
    {
      const uint64_t wn = std::min(window, nq - w0), ns = both ? 2 * wn : wn;
      const double t0 = now_s();
      VsxExactItem * items;
      if (host_all) { host_items.resize(ns); items = host_items.data(); }
      else { VSX_HIP_AS(WHO, ensure_pinned(X.h_items, ns)); items = X.h_items.p; }
      const Plan P = plan_items(wn, [&](uint64_t k) { return qlen[w0 + k]; }, both, hardq, items);
      char * text;
      if (host_all) { host_text.resize(P.text_bytes + 1); text = host_text.data(); }
      else { VSX_HIP_AS(WHO, ensure_pinned(X.h_text, P.text_bytes)); text = X.h_text.p; }
      fill_text(S, P, items, [&](uint64_t k) { return qblob + qoff[w0 + k]; }, text, hardq);
      g_stats.seconds_stage += now_s() - t0;

      Matches M {};
      if (host_all) host_window(X, P, items, text, lists, M);
      else { const int rc = device_window(S, X, P, M); if (rc != VSX_OK) return rc; }
      ++g_stats.windows;
      g_stats.strands_probed += ns;
      (host_all ? g_stats.queries_host : g_stats.queries_device) += wn;

      const double t1 = now_s();
      const uint64_t nb = (wn + per_block - 1) / per_block, base = blocks.size();
      for (uint64_t b = 0; b < nb; ++b) blocks.emplace_back(new Block);
      const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S->threads), nb));
      std::atomic<uint64_t> next {0};
      run_pool(nth, [&](int) {
        for (;;)
          {
            const uint64_t b = next.fetch_add(1);
            if (b >= nb) break;
            finish_queries(*S, P, M, b * per_block, std::min(wn, (b + 1) * per_block), w0, qlen, qmeta, *blocks[base + b]);
          }
      });
      for (uint64_t b = 0; b < nb; ++b)
        {
          const Block & B = *blocks[base + b];
          const Hit * p = B.hits.data();
          for (size_t k = 0; k < B.per_query.size(); ++k)
            {
              span[w0 + b * per_block + k] = HitSpan {p, B.per_query[k]};
              p += B.per_query[k];
              if (B.per_query[k]) ++g_stats.queries_matched;
            }
          g_stats.hits += B.hits.size();
        }
      g_stats.seconds_marshal += now_s() - t1;
    }
  const double t2 = now_s();
  const int rc = marshal_hits_from(nq, [&](uint64_t q) { return span[q]; }, out, S->threads);
  g_stats.seconds_marshal += now_s() - t2;
  return rc;
}

int check_queries(uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen, vsx_hits * out)
{
  if (!out || (nq && (!qblob || !qoff || !qlen))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (nq > (uint64_t) UINT32_MAX) return fail(VSX_EINVAL, "%s: more than UINT32_MAX queries", WHO);
  return vsxp::check_spans(WHO, "query", nq, qoff, qlen, qbytes);
}

}  // namespace

void vsx_internal_exact_index_destroy(VsxExactIndex * X)
{
  if (!X) return;
  if (X->ev_a) (void) hipEventDestroy(X->ev_a);
  if (X->ev_b) (void) hipEventDestroy(X->ev_b);
  delete X;
}

extern "C" {

void vsx_search_exact_last_stats(vsx_exact_stats * out) { if (out) *out = g_stats; }

int vsx_search_exact(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen,
                     const vsx_seq_meta * qmeta, vsx_hits * out)
{
  g_stats = vsx_exact_stats {};
  const double t_begin = now_s();
  if (!S) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const int rc_q = check_queries(nq, qblob, qbytes, qoff, qlen, out);
  if (rc_q != VSX_OK) return rc_q;
  const bool host_all = vsxp::env_is_host("VSX_EXACT") || !S->ctx;
  const int rc = run(S, host_all, nq, qblob, qoff, qlen, qmeta, out);
  if (rc != VSX_OK) { vsx_hits_free(out); return rc; }
  out->seconds_total = g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_search_exact_host(const vsx_scoring * scoring, const vsx_search_opts * opts, uint64_t n, const char * blob,
                                   uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths, const vsx_seq_meta * db_meta,
                                   uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen,
                                   const vsx_seq_meta * qmeta, vsx_hits * out)
{
  g_stats = vsx_exact_stats {};
  const double t_begin = now_s();
  if (!scoring || !opts || (n && (!blob || !offsets || !lengths))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const int rc_q = check_queries(nq, qblob, qbytes, qoff, qlen, out);
  if (rc_q != VSX_OK) return rc_q;
  if (opts->soft_mask < 0 || opts->soft_mask > 2 || opts->qmask < 0 || opts->qmask > 3 || opts->hardmask < 0 || opts->hardmask > 3)
    return fail(VSX_EINVAL, "%s: masking option out of range", WHO);
  if (const int rc = vsxp::check_spans(WHO, "sequence", n, offsets, lengths, blob_bytes)) return rc;
  // a searcher without a context: the text, the options and the annotations are all the host restatement reads
  vsx_searcher S;
  S.scoring = *scoring;
  S.o = *opts;
  if (S.o.weak_id > S.o.id) S.o.weak_id = S.o.id;
  S.blob.assign(blob, blob + blob_bytes);
  S.blob.push_back(0);
  S.off.assign(offsets, offsets + n);
  S.len.assign(lengths, lengths + n);
  S.threads = opts->threads > 0 ? opts->threads : vsxp::usable_cpus();
  S.qmode = S.o.qmask ? S.o.qmask - 1 : S.o.soft_mask;
  if ((S.o.hardmask & 1) && S.o.soft_mask != 0 && blob_bytes)
    {
      auto off = [&](uint64_t k) { return offsets[k]; };
      auto len = [&](uint64_t k) { return (int64_t) lengths[k]; };
      if (!sequences_disjoint(n, off, [&](uint64_t k) { return (uint64_t) lengths[k]; }))
        return fail(VSX_EINVAL, "%s: --hardmask needs sequences that do not overlap in the blob", WHO);
      if (S.o.soft_mask == 2) dust_states(&S, S.blob.data(), n, off, len, true);
      else hardmask_states(&S, S.blob.data(), n, off, len);
    }
  int rc = vsx_searcher_set_meta(&S, db_meta);
  if (rc == VSX_OK) rc = run(&S, true, nq, qblob, qoff, qlen, qmeta, out);
  vsx_internal_exact_index_destroy(S.xidx);
  S.xidx = nullptr;
  if (rc != VSX_OK) { vsx_hits_free(out); return rc; }
  out->seconds_total = g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
