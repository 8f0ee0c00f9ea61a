// vsx_search_internal.h -- what the four commands on a searcher share: vsx_search.cpp (the searcher, its index and filters,
// --usearch_global), vsx_allpairs.cpp (--allpairs_global), vsx_cluster.cpp (the clustering rounds) and vsx_denovo_search.cpp (the part
// search of de novo chimera detection).  Host-only C++, included by those four files alone.  The functions declared here are
// defined in vsx_search.cpp; the templates stay templates (their accessors are inlined into the per-query loops).
#ifndef VSX_SEARCH_INTERNAL_H
#define VSX_SEARCH_INTERNAL_H

#include "../../include/vsx_search.h"
#include "vsx_internal.h"
#include "vsx_kmer.h"
#include "vsx_private.h"

#include <algorithm>
#include <atomic>
#include <cinttypes>
#include <climits>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <condition_variable>
#include <mutex>
#include <vector>

// (hidden, as vsxp: nothing here adds to the library's dynamic symbols)
namespace vsxs __attribute__((visibility("hidden"))) {
// the query side of one searchinfo_s (core/searchcore.hpp:131-176) beyond the sequence: abundance, label
struct QMeta { int64_t qsize = 1; const char * label = nullptr; };
}  // namespace vsxs

struct vsx_searcher {
  vsx_ctx * ctx = nullptr;
  vsx_scoring scoring {};           // unclamped values, for the linear-memory fallback
  vsx_search_opts o {};
  std::vector<char> blob;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  vsx_seqset * dbset = nullptr;
  vsx_ctx * ctx2 = nullptr;          // a second aligner context of the same device (owned): the second consumer of the search pipeline
  vsx_ctx * ctx3 = nullptr;          // ... and the third
  int w = 8;
  int qmode = 0;                     // masking of raw queries: opts.qmask - 1, or opts.soft_mask when qmask == 0
  std::vector<uint64_t> kstart;      // 4^w + 1
  std::vector<uint32_t> postings;    // targets containing the k-mer, ascending
  int64_t ma = 1, mr = 32, tophits = 0, minwordmatches = 12;
  int threads = 1;
  bool indexed = false;              // the k-mer index is built on first use (allpairs never needs it)
  VsxKmerIndex * kidx = nullptr;     // device index (vsx_kmer.hip), built on first use by the batch search
  VsxExactIndex * xidx = nullptr;    // exact-match index (vsx_exact.cpp), built on first use by vsx_search_exact
  VsxSintaxIndex * sidx = nullptr;   // name ids of the labels and the window buffers of vsx_sintax (vsx_sintax.cpp), made on first use
  VsxOrientIndex * oidx = nullptr;   // match-count table and the window buffers of vsx_orient (vsx_orient.cpp), made on first use
  VsxHitoutIndex * hidx = nullptr;   // database text on the device and the window buffers of vsx_hits_render (vsx_hitout.cpp), made on first use
  std::vector<uint64_t> word_total;  // postings per word (statistics of the device index)
  std::vector<uint8_t> is_centroid;  // clustering: which sequences are in the growing index
  std::vector<uint64_t> tsize;       // Database::getabundance of the targets (empty: all 1)
  std::vector<std::string> tlabel;   // Database::getheader (empty: no labels, --self never fires)
  int64_t abundance(uint64_t seqno) const { return tsize.empty() ? 1 : (int64_t) tsize[seqno]; }
  // a database sequence in the query role (allpairs, clustering: si->qsize = db.getabundance, allpairs_global.cpp:398, cluster.cpp:176)
  vsxs::QMeta meta_of(uint64_t seqno) const { return vsxs::QMeta {abundance(seqno), tlabel.empty() ? nullptr : tlabel[seqno].c_str()}; }
};

namespace vsxs __attribute__((visibility("hidden"))) {

using vsxp::fail;
using vsxp::now_s;
using vsxp::run_pool;

// chrmap_complement, utils/maps.cpp:121-150, as vsx_symbols.h states it
inline char complement(unsigned char c) { return (char) vsxsym::complement(c); }

struct Cand { uint32_t target, count, length; };

// minheap order (core/minheap.cpp:111-146), best first: count desc, length asc, seqno asc
inline bool cand_better(const Cand & a, const Cand & b)
{
  if (a.count != b.count) return a.count > b.count;
  if (a.length != b.length) return a.length < b.length;
  return a.target < b.target;
}

struct Hit {
  uint32_t target = 0, count = 0;
  bool accepted = false, rejected = false, aligned = false, weak = false, fallback = false, minus = false;
  int nwscore = 0, nwdiff = 0, nwgaps = 0, nwindels = 0, nwalignmentlength = 0, matches = 0, mismatches = 0;
  int internal_alignmentlength = 0, internal_gaps = 0, internal_indels = 0;
  int trim_q_left = 0, trim_q_right = 0, trim_t_left = 0, trim_t_right = 0, trim_aln_left = 0, trim_aln_right = 0;
  int shortest = 0, longest = 0;
  double nwid = 0, id = 0, id0 = 0, id1 = 0, id2 = 0, id3 = 0, id4 = 0;
  std::string cigar;
};

struct QState {
  std::vector<Cand> cands;      // best first
  size_t next = 0;
  std::vector<Hit> hits;        // si->hits[0 .. hit_count)
  int64_t accepts = 0, rejects = 0, finalized = 0;
  int delayed = 0;
  int lazy_first = 0;           // lazy search: delayed candidates of the (short) first batch; the second batch completes the reference's eight
  bool done = false;
  uint64_t req_first = 0;       // first pair of this query's pending batch in the stage plan
  uint32_t req_count = 0;
};

// Growing index used by clustering: only centroids are indexed (Dbindex::add_sequence, core/dbindex.cpp:125-152)
struct IncIndex {
  std::vector<std::vector<uint32_t>> post;      // k-mer -> centroid sequence numbers, ascending
  uint64_t indexed = 0;
};

struct Acct { double t_align = 0, t_advance = 0, t_replay = 0; uint64_t pairs = 0, cells = 0, stages = 0, sentinels = 0; };
struct KmerAcct { double kernel_ms = 0, build_ms = 0; uint64_t streamed = 0, streamed_bytes = 0, postings = 0; bool want_streamed = false; };      // want_streamed: count the postings a batch streams (a serial pass over its words: benches only)

// ---- defined in vsx_search.cpp ----
// the size, in 64-bit words, of the `seen` scratch bitmap unique_kmers wants (4^w bits for w < 10, unused beyond)
inline size_t seen_words(const vsx_searcher & S) { return S.w < 10 ? (size_t) (((1ull << (2 * S.w)) + 63) / 64) : 1; }
void unique_kmers(const char * seq, int64_t len, int w, bool soft, std::vector<uint32_t> & out, std::vector<uint64_t> & seen);
void build_index(vsx_searcher * S);
void candidates_for(const vsx_searcher & S, const char * q, int64_t qlen, std::vector<uint16_t> & counts,
                    std::vector<uint32_t> & touched, std::vector<uint32_t> & kmers, std::vector<uint64_t> & seen,
                    std::vector<Cand> & out, const IncIndex * inc = nullptr);
bool acceptable_unaligned(const vsx_searcher & S, const char * q, int64_t qlen, uint32_t target, const QMeta & qm = QMeta {});
bool acceptable_aligned(const vsx_searcher & S, int64_t qlen, Hit & h, int64_t qsize = 1);
bool advance(const vsx_searcher & S, QState & st, const char * q, int64_t qlen, uint32_t qlocal, const QMeta & qm,
             std::vector<uint32_t> & pq, std::vector<uint32_t> & pt, bool lazy);
void align_trim(Hit & h, int iddef);
vsx_filter make_filter(const vsx_searcher & S);
void hit_record(const Hit & h, uint32_t q, uint64_t cigar_off, vsx_hit & o);
int hit_compare_byid(const Hit & l, const Hit & r);
int hit_compare_bysize(const vsx_searcher & S, const Hit & l, const Hit & r);
bool device_kmer_ok(const vsx_searcher & S);
bool device_kmer_subsets_ok(const vsx_searcher & S);
int device_rank(const vsx_searcher * S, VsxKmerIndex * ix, const std::vector<uint32_t> * map, uint64_t nq,
                const std::vector<std::vector<uint32_t>> & words, uint32_t keep, uint32_t cap_hint, bool rank,
                std::vector<std::vector<Cand>> & cands, std::vector<uint64_t> & fallback, KmerAcct & acct,
                int thread_cap = 0 /* > 0: the caller runs beside other helpers and owns only this share of S->threads */);
// the three blocks of a vsx_hits for nq queries (sizes and counts filled in, nothing else); VSX_ENOMEM leaves *out freed and zeroed
int alloc_hits(vsx_hits * out, uint64_t nq, uint64_t n_hits, uint64_t cigar_bytes);
int marshal_hits(std::vector<std::vector<Hit>> & kept, vsx_hits * out, int thread_budget);

// ---- the templates ----
// Fill a hit from one alignment result (searchcore.cpp:806-857 == allpairs_global.cpp:447-508): linear-memory
// fallback on the sentinel, derived fields, align_trim.  Returns VSX_OK or an error code.
// (qtext() yields the query as text; it is only called on the sentinel path -- minus-strand queries have no text otherwise)
template <typename FQ>
int fill_hit(const vsx_searcher & S, FQ qtext, int64_t ql, Hit & h, const vsx_results & res, uint64_t r,
                    uint64_t & sentinels)
{
  int64_t alnlen = res.aligned[r], nm = res.matches[r], nmm = res.mismatches[r];
  int64_t nwscore = res.score[r], nwgaps = res.gaps[r];
  const int64_t dl = S.len[h.target];
  if (res.score[r] == VSX_SCORE_SENTINEL)
    {
      ++sentinels;
      char * cg = nullptr;
      const int rc = vsx_lma_align(&S.scoring, qtext(), (uint64_t) ql, S.blob.data() + S.off[h.target], (uint64_t) dl,
                                   &nwscore, &alnlen, &nm, &nmm, &nwgaps, &cg);
      if (rc != VSX_OK) return rc;
      h.cigar = cg;
      std::free(cg);
      h.fallback = true;
    }
  else h.cigar = res.cigar_blob + res.cigar_off[r];
  h.aligned = true;
  h.shortest = (int) std::min<int64_t>(ql, dl);
  h.longest = (int) std::max<int64_t>(ql, dl);
  h.nwscore = (int) nwscore;
  h.nwdiff = (int) (alnlen - nm);
  h.nwgaps = (int) nwgaps;
  h.nwindels = (int) (alnlen - nm - nmm);
  h.nwalignmentlength = (int) alnlen;
  h.nwid = 100.0 * (double) (alnlen - h.nwdiff) / (double) alnlen;
  h.matches = (int) (alnlen - h.nwdiff);
  h.mismatches = h.nwdiff - h.nwindels;
  align_trim(h, S.o.iddef);
  return VSX_OK;
}

// (range_of(q) -> the hits of query q as a span; r06: the search keeps a window's hits in ONE vector -- a vector per query was 10^5 small
//  blocks allocated on the consumer threads and released on the caller's at return: 8-11 ms of a 130 ms call)
struct HitSpan { const Hit * p; size_t n; const Hit * begin() const { return p; } const Hit * end() const { return p + n; } size_t size() const { return n; } };
template <typename FRange>
int marshal_hits_from(uint64_t nq, FRange range_of, vsx_hits * out, int thread_budget /* the searcher's: S->threads */)
{
  // positions first (a serial scan over two numbers per query), then the copies on host threads (r04: the serial form was 4-5 ms of a
  // 140 ms search call of 100 k queries)
  std::vector<uint64_t> first_at(nq + 1), blob_at(nq + 1);
  uint64_t total = 0, bytes = 0;
  for (uint64_t q = 0; q < nq; ++q)
    {
      first_at[q] = total;
      blob_at[q] = bytes;
      const HitSpan sp = range_of(q);
      total += sp.size();
      for (const Hit & h : sp) bytes += h.cigar.size() + 1;
    }
  first_at[nq] = total;
  blob_at[nq] = bytes;
  const int arc = alloc_hits(out, nq, total, bytes);
  if (arc != VSX_OK) return arc;
  std::memcpy(out->first, first_at.data(), (nq + 1) * sizeof(uint64_t));
  auto fill = [&](uint64_t q0, uint64_t q1) {
    for (uint64_t q = q0; q < q1; ++q)
      {
        uint64_t pos = out->first[q], at = blob_at[q];
        for (const Hit & h : range_of(q))
          {
            vsx_hit & o = out->hit[pos++];
            hit_record(h, (uint32_t) q, at, o);
            std::memcpy(out->cigar_blob + at, h.cigar.data(), h.cigar.size());
            at += h.cigar.size();
            out->cigar_blob[at++] = '\0';
          }
      }
  };
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::min(std::max(1, thread_budget), 8), total / 16384));
  if (nth <= 1) fill(0, nq);
  else
    {
      std::vector<std::thread> pool;
      for (int t = 1; t < nth; ++t) pool.emplace_back(fill, nq * (uint64_t) t / (uint64_t) nth, nq * (uint64_t) (t + 1) / (uint64_t) nth);
      fill(0, nq / (uint64_t) nth);
      for (std::thread & t : pool) t.join();
    }
  return VSX_OK;
}
// The staged search of a window: every open query contributes its next align_delayed batch, all batches go to the
// GPU as one plan, then the reference's bookkeeping (:782-878) is replayed per query.  qseq/qlen/qidx map a window
// slot to its sequence, length and index inside `qset`.
// qseq(k): the query for the symbol-comparing filters (only dereferenced when idprefix / idsuffix / selfid are set);
// qtext(k): the query as text for the linear-memory fallback (sentinel pairs only; may build it on demand).
template <typename FSeq, typename FText, typename FLen, typename FIdx, typename FMeta>
int run_stages(const vsx_searcher & S, std::vector<QState> & st, FSeq qseq, FText qtext, FLen qlen, FIdx qidx, FMeta qmeta,
                      const vsx_seqset * qset, Acct & acct, vsx_ctx * ctx = nullptr /* default: the searcher's own */, bool lazy = false)
{
  if (!ctx) ctx = S.ctx;
  const uint64_t wn = st.size();
  std::vector<uint32_t> open(wn);
  for (uint64_t k = 0; k < wn; ++k) open[k] = (uint32_t) k;
  std::vector<uint32_t> pq, pt;
  while (!open.empty())
    {
      pq.clear(); pt.clear();
      std::vector<uint32_t> waiting;
      const double ta = now_s();
      {
        // every open query up to its next align_delayed batch: contiguous slices of `open` on host threads, concatenated
        // in order (the pair list, and with it every result, is independent of the thread count)
        const int nth = (int) std::max<size_t>(1, std::min<size_t>((size_t) std::max(1, S.threads), open.size() / 512));
        struct Part { std::vector<uint32_t> pq, pt, waiting; };
        std::vector<Part> part((size_t) nth);
        auto work = [&](int t) {
          Part & p = part[(size_t) t];
          const size_t b = open.size() * (size_t) t / (size_t) nth, e = open.size() * (size_t) (t + 1) / (size_t) nth;
          for (size_t w = b; w < e; ++w)
            {
              const uint32_t k = open[w];
              if (advance(S, st[k], qseq(k), qlen(k), qidx(k), qmeta(k), p.pq, p.pt, lazy)) p.waiting.push_back(k);     // req_first: slice-relative
            }
        };
        run_pool(nth, work);
        for (int t = 0; t < nth; ++t)
          {
            Part & p = part[(size_t) t];
            const uint64_t base = pq.size();
            for (uint32_t k : p.waiting) st[k].req_first += base;
            pq.insert(pq.end(), p.pq.begin(), p.pq.end());
            pt.insert(pt.end(), p.pt.begin(), p.pt.end());
            waiting.insert(waiting.end(), p.waiting.begin(), p.waiting.end());
          }
      }
      acct.t_advance += now_s() - ta;
      if (waiting.empty()) break;
      ++acct.stages;
      const double t0 = now_s();
      vsx_results res;
      const vsx_filter flt = make_filter(S);
      // with '*' penalties every pair takes the linear-memory fallback and the forbidden-gap test, and the UNOISE rule needs the
      // abundances: nothing for the device to decide
      int rc = vsx_align_pairs_filtered(ctx, qset, S.dbset, pq.size(), pq.data(), pt.data(),
                                        (S.o.gap_infinite || S.o.cluster_unoise) ? nullptr : &flt, &res);
      acct.t_align += now_s() - t0;
      if (rc != VSX_OK) return rc;
      acct.pairs += pq.size();
      // the reference's bookkeeping per query (:782-878), host threads over the queries of the stage
      const double tr = now_s();
      {
        const int nth = (int) std::max<size_t>(1, std::min<size_t>((size_t) std::max(1, S.threads), waiting.size() / 256));
        std::vector<Acct> part((size_t) nth);
        std::vector<int> err((size_t) nth, VSX_OK);
        std::atomic<size_t> next {0};
        auto work = [&](int tid) {
          Acct & a = part[(size_t) tid];
          for (;;)
            {
              const size_t b = next.fetch_add(64);
              if (b >= waiting.size()) break;
              const size_t e = std::min(waiting.size(), b + 64);
              for (size_t w = b; w < e; ++w)
                {
                  const uint32_t k = waiting[w];
                  QState & q = st[k];
                  const int64_t ql = qlen(k);
                  uint64_t i = q.req_first;
                  for (size_t x = (size_t) q.finalized; x < q.hits.size(); ++x)
                    {
                      Hit & h = q.hits[x];
                      const bool live = (q.rejects < S.mr) && (q.accepts < S.ma);
                      if (h.rejected) { if (live) ++q.rejects; continue; }
                      const uint64_t r = i++;
                      a.cells += (uint64_t) ql * S.len[h.target];
                      if (!live) continue;                                   // ignored hit: stays unaligned (:785, :875-878)
                      const uint8_t verdict = res.verdict ? res.verdict[r] : (uint8_t) VSX_VERDICT_UNDECIDED;
                      if (verdict == VSX_VERDICT_REJECTED)
                        {
                          // decided on the device (align_trim + search_acceptable_aligned): not reported, no CIGAR fetched
                          h.aligned = true; h.rejected = true; h.weak = false;
                          ++q.rejects;
                          continue;
                        }
                      const int frc = fill_hit(S, [&]() { return qtext(k); }, ql, h, res, r, a.sentinels);
                      if (frc != VSX_OK) { err[(size_t) tid] = frc; return; }
                      const bool acc = acceptable_aligned(S, ql, h, qmeta(k).qsize);
                      if (verdict != VSX_VERDICT_UNDECIDED && (acc != (verdict == VSX_VERDICT_ACCEPTED) || (!acc && !h.weak)))
                        { err[(size_t) tid] = VSX_EHIP; return; }
                      if (acc) ++q.accepts; else ++q.rejects;
                    }
                  q.finalized = (int64_t) q.hits.size();
                  q.delayed = 0;
                }
            }
        };
        run_pool(nth, work);
        for (int t = 0; t < nth; ++t)
          {
            acct.cells += part[(size_t) t].cells; acct.sentinels += part[(size_t) t].sentinels;
            if (err[(size_t) t] != VSX_OK)
              {
                vsx_results_free(&res);
                return fail(err[(size_t) t], err[(size_t) t] == VSX_EHIP ? "search: device and host accept filters disagree"
                                                                           : "search: fallback aligner failed");
              }
          }
      }
      acct.t_replay += now_s() - tr;
      vsx_results_free(&res);
      open.swap(waiting);
    }
  return VSX_OK;
}

// DUST rewrites the text in place (host threads per sequence, atomicOr on the device): sequences that share bytes of the blob would
// race and come out with the union of their masks, unlike the reference's per-sequence dust().  Offsets in ascending order (every
// caller of ours) cost one sweep; anything else is sorted first.
template <typename FOff, typename FLen>
bool sequences_disjoint(uint64_t n, FOff off, FLen len)
{
  bool ascending = true;
  uint64_t end = 0;
  for (uint64_t k = 0; k < n && ascending; ++k)
    {
      const uint64_t o = off(k), l = len(k);
      if (l == 0) continue;
      if (o < end) ascending = false;
      end = o + l;
    }
  if (ascending) return true;
  std::vector<std::pair<uint64_t, uint64_t>> iv;
  iv.reserve(n);
  for (uint64_t k = 0; k < n; ++k) if (len(k)) iv.emplace_back(off(k), off(k) + len(k));
  std::sort(iv.begin(), iv.end());
  for (size_t k = 1; k < iv.size(); ++k) if (iv[k].first < iv[k - 1].second) return false;
  return true;
}

// DUST of raw queries (query masking mode 2): the reference masks every query -- and each strand of it separately -- in place before
// anything else reads it (core/search.cpp:294-303, commands/usearch_global.cpp:386-392); text[off(k) .. + len(k)) for k < n.
// The sequences must not overlap in the blob (sequences_disjoint; the callers check).
template <typename FOff, typename FLen>
void dust_states(const vsx_searcher * S, char * text, uint64_t n, FOff off, FLen len, bool hard = false)
{
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S->threads), n / 32 + 1));
  std::atomic<uint64_t> next {0};
  auto work = [&]() {
    std::vector<char> scratch;
    for (;;)
      {
        const uint64_t k0 = next.fetch_add(32);
        if (k0 >= n) break;
        for (uint64_t k = k0; k < std::min(n, k0 + 32); ++k) vsx_internal_dust_one(text + off(k), (int64_t) len(k), scratch, hard);
      }
  };
  run_pool(nth, [&](int) { work(); });
}
// --hardmask with soft masking (core/mask.cpp:248-271): every lower-case symbol -- bit 0x20 set -- becomes 'N'
template <typename FOff, typename FLen>
void hardmask_states(const vsx_searcher * S, char * text, uint64_t n, FOff off, FLen len)
{
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S->threads), n / 256 + 1));
  std::atomic<uint64_t> next {0};
  run_pool(nth, [&](int) {
    for (;;)
      {
        const uint64_t k0 = next.fetch_add(256);
        if (k0 >= n) break;
        for (uint64_t k = k0; k < std::min(n, k0 + 256); ++k)
          {
            char * p = text + off(k);
            const uint64_t L = (uint64_t) len(k);
            for (uint64_t i = 0; i < L; ++i) if (((unsigned char) p[i] & 0x20u) != 0u) p[i] = 'N';
          }
      }
  });
}

// device path of search_topscores, stage 1: unique words per query (host threads; unique_count, core/unique.cpp:155-352)
template <typename FSeq, typename FLen>
void kmer_words(const vsx_searcher * S, uint64_t nq, FSeq qseq, FLen qlen, std::vector<std::vector<uint32_t>> & words)
{
  const int nth = std::max(1, S->threads);
  const uint64_t nwords = 1ull << (2 * S->w);
  words.assign(nq, {});
  std::vector<std::vector<uint64_t>> seen((size_t) nth, std::vector<uint64_t>((nwords + 63) / 64, 0));
  std::atomic<uint64_t> next {0};
  auto work = [&](int tid) {
    for (;;)
      {
        const uint64_t k = next.fetch_add(1);
        if (k >= nq) break;
        unique_kmers(qseq(k), qlen(k), S->w, S->qmode != 0, words[k], seen[(size_t) tid]);
      }
  };
  run_pool(nth, work);
}

// stage 2: count on the device index (built on first use), threshold, rank; queries the 16-bit counters cannot serve go
// through the host restatement
template <typename FSeq, typename FLen>
int kmer_rank(vsx_searcher * S, uint64_t nq, FSeq qseq, FLen qlen, const std::vector<std::vector<uint32_t>> & words,
                     std::vector<std::vector<Cand>> & cands, KmerAcct & acct)
{
  static const bool kdebug = std::getenv("VSX_KMER_DEBUG") != nullptr;
  cands.assign(nq, {});
  static std::mutex once_mu;                           // two windows' k-mer stages may run at once (vsx_search_batch)
  {
    std::lock_guard<std::mutex> lk(once_mu);
    if (!S->kidx)
      {
        const int rc = vsx_kmer_index_create(S->ctx, S->dbset, S->w, &S->kidx);
        if (rc != VSX_OK) return rc;
        acct.build_ms = vsx_kmer_stats(S->kidx)->build_ms;
      }
    acct.postings = vsx_kmer_stats(S->kidx)->postings;
  }
  std::vector<uint64_t> fallback;
  const double tw1 = now_s();
  {
    const int rc = device_rank(S, S->kidx, nullptr, nq, words, (uint32_t) std::max<int64_t>(S->tophits, 1), 0, true, cands, fallback, acct);
    if (rc != VSX_OK) return rc;
  }
  if (kdebug) std::fprintf(stderr, "kmer_rank: %llu queries: %.3f s\n", (unsigned long long) nq, now_s() - tw1);
  if (!fallback.empty())
    {
      std::lock_guard<std::mutex> lk(once_mu);         // the host index is built on first use
      build_index(S);
      std::vector<uint16_t> counts(S->len.size(), 0);
      std::vector<uint32_t> touched, km;
      std::vector<uint64_t> seen(seen_words(*S), 0);
      for (uint64_t k : fallback) candidates_for(*S, qseq(k), qlen(k), counts, touched, km, seen, cands[k]);
    }
  return VSX_OK;
}

// search_topscores for a batch: cands[k] = candidate list of query k, best first, <= tophits entries.
template <typename FSeq, typename FLen>
int batch_candidates(vsx_searcher * S, bool device, uint64_t nq, FSeq qseq, FLen qlen,
                            std::vector<std::vector<Cand>> & cands, KmerAcct & acct)
{
  cands.assign(nq, {});
  const int nth = std::max(1, S->threads);
  auto parallel = [&](auto && fn) {
    std::atomic<uint64_t> next {0};
    auto work = [&](int tid) { for (;;) { const uint64_t k = next.fetch_add(1); if (k >= nq) break; fn(tid, k); } };
    run_pool(nth, work);
  };

  if (!device)
    {
      build_index(S);
      struct Scratch { std::vector<uint16_t> counts; std::vector<uint32_t> touched, km; std::vector<uint64_t> seen; };
      std::vector<Scratch> scratch((size_t) nth);
      for (auto & sc : scratch)
        {
          sc.counts.assign(S->len.size(), 0);
          sc.seen.assign(seen_words(*S), 0);
        }
      parallel([&](int tid, uint64_t k) {
        Scratch & sc = scratch[(size_t) tid];
        candidates_for(*S, qseq(k), qlen(k), sc.counts, sc.touched, sc.km, sc.seen, cands[k]);
      });
      return VSX_OK;
    }

  std::vector<std::vector<uint32_t>> words;
  kmer_words(S, nq, qseq, qlen, words);
  return kmer_rank(S, nq, qseq, qlen, words, cands, acct);
}

}  // namespace vsxs

#endif
