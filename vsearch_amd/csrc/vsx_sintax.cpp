// vsx_sintax.cpp -- SINTAX taxonomy classification (include/vsx_sintax.h), the host side of vsx_sintax.hip.
//
// Restated from the reference (src/):
//   sintax_query / sintax_search_topscores / sintax_analyse   commands/sintax.cpp   rounds, winner, strand choice, vote
//   tax_parse / tax_split                                     core/tax.cpp          where the nine rank names lie in a header
//   SplitMix64 / random_substream_seed / random_bounded       utils/random.{hpp,cpp}  (vsx_sintax_internal.h, shared with the kernels)
//   unique_count (Masking::none)                              core/unique.cpp       a strand's words in first-occurrence order
//
// A device call runs its queries in windows: host threads build both strands' word lists (CSR, pinned), the sample kernel
// draws every round's words, the count kernel leaves one key per (round, tile), the vote kernel returns the record.  The host
// restatement does the same per query with one counter per database sequence over the searcher's host index; it is the only
// place that knows --sintax_random (a reservoir draw per database sequence in scan order).
#include "vsx_search_internal.h"
#include "vsx_sintax_internal.h"
#include "vsx_tax_split.h"

#include <unordered_map>
#include <unordered_set>

using namespace vsxs;
using vsxp::DevBuf;
using vsxp::PinnedBuf;
using vsxp::ensure_pinned;
using vsxp::map4;

#define WHO "vsx_sintax"

struct VsxSintaxIndex {
  // the name ids of the database labels, N x 9 (host; device copy made by the first device call)
  bool tax_ready = false;
  std::vector<uint32_t> taxid;
  bool device_ready = false;
  DevBuf<uint32_t> d_taxid;
  // the window's buffers (grow-only, kept between calls)
  PinnedBuf<uint64_t> h_wstart, h_qno;
  PinnedBuf<uint32_t> h_words, h_cand;
  PinnedBuf<SxVote> h_vote;
  DevBuf<uint64_t> d_wstart, d_qno, d_keys;
  DevBuf<uint32_t> d_words, d_samples, d_cand;
  DevBuf<uint8_t> d_nsample;
  DevBuf<SxVote> d_vote;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

namespace {

thread_local vsx_sintax_stats g_stats;

using vsxtax::tax_split;                                          // tax_parse + tax_split (core/tax.cpp:70-186), vsx_tax_split.h

// ids[9 i + k]: 0 = the empty name; equal iff (length, bytes) are equal
void intern_labels(uint64_t n, const char * const * labels, uint32_t * ids, int32_t * start_out, int32_t * len_out)
{
  std::unordered_map<std::string, uint32_t> seen[SX_RANKS];
  for (int k = 0; k < SX_RANKS; ++k) seen[k].emplace(std::string(), 0u);
  for (uint64_t i = 0; i < n; ++i)
    {
      const char * h = labels[i] ? labels[i] : "";
      int st[SX_RANKS], ln[SX_RANKS];
      tax_split(h, (int) std::strlen(h), st, ln);
      for (int k = 0; k < SX_RANKS; ++k)
        {
          const auto it = seen[k].emplace(std::string(h + st[k], (size_t) ln[k]), (uint32_t) seen[k].size());
          ids[i * SX_RANKS + (uint64_t) k] = it.first->second;
          if (start_out) start_out[i * SX_RANKS + (uint64_t) k] = st[k];
          if (len_out) len_out[i * SX_RANKS + (uint64_t) k] = ln[k];
        }
    }
}

// unique_count with Masking::none (core/unique.cpp:155-352): the distinct words of a strand in the order they first occur;
// only a symbol outside ACGTU (either case) poisons the words that cover it.  minus: the reverse complement is read.
struct WordScratch { std::vector<uint64_t> seen; std::unordered_set<uint32_t> set; };
void strand_words(const char * seq, int64_t len, int w, bool minus, std::vector<uint32_t> & out, WordScratch & sc)
{
  out.clear();
  const uint64_t mask = (1ull << (2 * w)) - 1;
  const bool bitmap = w < 10;
  if (bitmap && sc.seen.size() < (mask >> 6) + 1) sc.seen.assign((mask >> 6) + 1, 0);
  if (!bitmap) sc.set.clear();
  uint64_t bad = 0, kmer = 0;
  for (int64_t s = 0; s < len; ++s)
    {
      const unsigned char c = minus ? (unsigned char) complement((unsigned char) seq[len - 1 - s]) : (unsigned char) seq[s];
      const uint8_t c4 = map4(c);
      const bool amb = vsxp::ambiguous4(c4);
      bad = ((bad << 2) | (amb ? 1u : 0u)) & mask;
      kmer = ((kmer << 2) | (amb ? 0u : (uint64_t) ((c4 >> 1) - (c4 >> 3)))) & mask;
      if (s < w - 1 || bad) continue;
      if (bitmap)
        {
          uint64_t & word = sc.seen[kmer >> 6];
          const uint64_t bit = 1ull << (kmer & 63);
          if (!(word & bit)) { word |= bit; out.push_back((uint32_t) kmer); }
        }
      else if (sc.set.insert((uint32_t) kmer).second) out.push_back((uint32_t) kmer);
    }
  if (bitmap) for (uint32_t k : out) sc.seen[k >> 6] = 0;
}

// one round's draws: 32 indices into the strand's K words, a repeated index dropped
int sample_round(uint64_t & state, const std::vector<uint32_t> & words, uint32_t * sample)
{
  uint32_t taken[SX_SUBSET];
  int n = 0;
  for (int j = 0; j < SX_SUBSET; ++j)
    {
      const uint32_t x = (uint32_t) sx_bounded(state, words.size());
      bool dup = false;
      for (int i = 0; i < n; ++i) dup = dup || taken[i] == x;
      if (!dup) { taken[n] = x; sample[n++] = words[x]; }
    }
  return n;
}

// sintax_analyse's vote over the chosen strand's candidates
void vote(const uint32_t * cand, uint32_t count, const uint32_t * taxid, vsx_sintax_record & rec)
{
  bool incl[SX_ROUNDS];
  for (uint32_t i = 0; i < count; ++i) incl[i] = true;
  for (int k = 0; k < SX_RANKS; ++k)
    {
      int match[SX_ROUNDS], members[SX_ROUNDS];
      for (uint32_t i = 0; i < count; ++i) { match[i] = -1; members[i] = 0; }
      for (uint32_t i = 0; i < count; ++i)
        if (incl[i])
          for (uint32_t j = 0; j <= i; ++j)
            if (incl[j] && taxid[(size_t) cand[i] * SX_RANKS + (size_t) k] == taxid[(size_t) cand[j] * SX_RANKS + (size_t) k])
              {
                match[i] = (int) j;
                ++members[j];
                break;
              }
      int best = -1, most = 0;
      for (uint32_t i = 0; i < count; ++i) if (members[i] > most) { best = (int) i; most = members[i]; }
      for (uint32_t i = 0; i < count; ++i) if (match[i] != best) incl[i] = false;
      rec.rank_seq[k] = best >= 0 ? cand[best] : VSX_SINTAX_NONE;
      rec.rank_count[k] = (uint32_t) most;
    }
}

struct HostScratch {
  std::vector<uint8_t> counts;
  std::vector<uint32_t> touched, words;
  WordScratch ws;
};

// sintax_query for one query on the searcher's host index
void host_query(const vsx_searcher & S, const VsxSintaxIndex & X, const vsx_sintax_opts & o, const char * q, int64_t ql, uint64_t qno,
                HostScratch & sc, vsx_sintax_record & rec, uint32_t * cand_out)
{
  const uint64_t n = S.len.size();
  uint32_t cand[2][SX_ROUNDS];
  std::memset(&rec, 0, sizeof rec);
  uint64_t state = sx_substream(o.randseed, qno);
  if (sc.counts.size() < n) sc.counts.assign(n, 0);
  for (int s = 0; s < (o.strand_both ? 2 : 1); ++s)
    {
      strand_words(q, ql, S.w, s != 0, sc.words, sc.ws);
      if (sc.words.size() < SX_SUBSET) continue;
      for (int r = 0; r < SX_ROUNDS; ++r)
        {
          uint32_t sample[SX_SUBSET];
          const int ns = sample_round(state, sc.words, sample);
          sc.touched.clear();
          for (int x = 0; x < ns; ++x)
            for (uint64_t p = S.kstart[sample[x]]; p < S.kstart[(size_t) sample[x] + 1]; ++p)
              {
                const uint32_t t = S.postings[p];
                if (sc.counts[t]++ == 0) sc.touched.push_back(t);
              }
          uint32_t bc = 0, bs = 0, bl = 0;
          if (o.sintax_random)
            {
              // every database sequence in scan order; a tie -- also at count 0 against the initial best -- draws from the stream
              uint64_t ties = 0;
              for (uint64_t i = 0; i < n; ++i)
                {
                  const uint32_t c = sc.counts[i];
                  if (c > bc) { bc = c; bs = (uint32_t) i; bl = S.len[i]; ties = 1; }
                  else if (c == bc)
                    {
                      ++ties;
                      if (sx_bounded(state, ties) == 0) { bs = (uint32_t) i; bl = S.len[i]; }
                    }
                }
            }
          else
            for (const uint32_t t : sc.touched)                      // count desc, length asc, number asc: the order of the scan cannot matter
              {
                const uint32_t c = sc.counts[t], l = S.len[t];
                if (c > bc || (c == bc && (l < bl || (l == bl && t < bs)))) { bc = c; bs = t; bl = l; }
              }
          for (const uint32_t t : sc.touched) sc.counts[t] = 0;
          if (bc > 1)
            {
              cand[s][rec.boot_count[s]++] = bs;
              rec.best_count[s] = std::max(rec.best_count[s], bc);
            }
        }
    }
  int strand = 0;
  if (o.strand_both)
    {
      if (rec.best_count[0] > rec.best_count[1]) strand = 0;
      else if (rec.best_count[1] > rec.best_count[0]) strand = 1;
      else strand = rec.boot_count[0] >= rec.boot_count[1] ? 0 : 1;
    }
  rec.strand = strand;
  rec.classified = rec.boot_count[strand] >= (SX_ROUNDS + 1) / 2 ? 1 : 0;
  if (rec.classified) vote(cand[strand], rec.boot_count[strand], X.taxid.data(), rec);
  else for (int k = 0; k < SX_RANKS; ++k) { rec.rank_seq[k] = VSX_SINTAX_NONE; rec.rank_count[k] = 0; }
  if (cand_out)
    for (int s = 0; s < 2; ++s)
      for (uint32_t i = 0; i < SX_ROUNDS; ++i) cand_out[s * SX_ROUNDS + (int) i] = i < rec.boot_count[s] ? cand[s][i] : VSX_SINTAX_NONE;
}

struct Queries {
  uint64_t n; const char * blob; const uint64_t * off; const uint32_t * len; uint64_t first_no; const uint64_t * no;
  uint64_t number(uint64_t k) const { return no ? no[k] : first_no + k; }
};

void run_host(vsx_searcher * S, VsxSintaxIndex & X, const vsx_sintax_opts & o, const Queries & Q, vsx_sintax_result * out)
{
  const double t0 = now_s();
  build_index(S);
  g_stats.seconds_index += now_s() - t0;
  const double t1 = now_s();
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S->threads), Q.n));
  std::vector<HostScratch> scratch((size_t) nth);
  std::atomic<uint64_t> next {0};
  run_pool(nth, [&](int tid) {
    for (;;)
      {
        const uint64_t k = next.fetch_add(1);
        if (k >= Q.n) break;
        host_query(*S, X, o, Q.blob + Q.off[k], (int64_t) Q.len[k], Q.number(k), scratch[(size_t) tid], out->rec[k],
                   out->candidates ? out->candidates + k * 2 * SX_ROUNDS : nullptr);
      }
  });
  g_stats.seconds_count += now_s() - t1;
}

int ensure_device(vsx_searcher * S, VsxSintaxIndex & X)
{
  const double t0 = now_s();
  if (!S->kidx)
    {
      const int rc = vsx_kmer_index_create(S->ctx, S->dbset, S->w, &S->kidx);
      if (rc != VSX_OK) return rc;
    }
  if (!X.device_ready)
    {
      VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
      hipStream_t st = vsx_internal_stream(S->ctx);
      for (auto & e : X.ev) VSX_HIP_AS(WHO, hipEventCreate(&e));
      VSX_HIP_AS(WHO, X.d_taxid.alloc(X.taxid.size()));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_taxid.p, X.taxid.data(), X.taxid.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      X.device_ready = true;
    }
  g_stats.seconds_index += now_s() - t0;
  return VSX_OK;
}

int run_device(vsx_searcher * S, VsxSintaxIndex & X, const vsx_sintax_opts & o, const Queries & Q, vsx_sintax_result * out)
{
  const int rc0 = ensure_device(S, X);
  if (rc0 != VSX_OK) return rc0;
  VsxKmerView V;
  const int rcv = vsx_kmer_index_view(S->kidx, &V);
  if (rcv != VSX_OK) return rcv;
  if (!V.packed || V.nseq != S->len.size()) return fail(VSX_EHIP, "%s: the searcher's k-mer index is not the packed whole-set index", WHO);
  const uint8_t * d_codes; const uint64_t * d_off; const uint32_t * d_len; uint64_t n_all;
  vsx_internal_seqset_device(S->dbset, &d_codes, &d_off, &d_len, &n_all);
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
  hipStream_t st = vsx_internal_stream(S->ctx);
  const uint64_t window = o.window > 0 ? (uint64_t) o.window : 4096;
  const int nth = std::max(1, S->threads);
  std::vector<std::vector<uint32_t>> lists;
  std::vector<WordScratch> ws((size_t) nth);

  for (uint64_t w0 = 0; w0 < Q.n; w0 += window)
    {
      const uint64_t wn = std::min(window, Q.n - w0), nl = 2 * wn;
      // ---- stage: both strands' word lists on host threads, then one CSR
      const double t0 = now_s();
      lists.resize(nl);
      {
        std::atomic<uint64_t> next {0};
        run_pool((int) std::min<uint64_t>((uint64_t) nth, wn), [&](int tid) {
          for (;;)
            {
              const uint64_t k = next.fetch_add(16);
              if (k >= wn) break;
              for (uint64_t x = k; x < std::min(wn, k + 16); ++x)
                for (int s = 0; s < 2; ++s)
                  {
                    if (s && !o.strand_both) { lists[2 * x + 1].clear(); continue; }
                    strand_words(Q.blob + Q.off[w0 + x], (int64_t) Q.len[w0 + x], S->w, s != 0, lists[2 * x + (uint64_t) s], ws[(size_t) tid]);
                  }
            }
        });
      }
      VSX_HIP_AS(WHO, ensure_pinned(X.h_wstart, nl + 1));
      VSX_HIP_AS(WHO, ensure_pinned(X.h_qno, wn));
      uint64_t total = 0;
      for (uint64_t l = 0; l < nl; ++l) { X.h_wstart.p[l] = total; total += lists[l].size(); }
      X.h_wstart.p[nl] = total;
      VSX_HIP_AS(WHO, ensure_pinned(X.h_words, total));
      for (uint64_t l = 0; l < nl; ++l) if (!lists[l].empty()) std::memcpy(X.h_words.p + X.h_wstart.p[l], lists[l].data(), lists[l].size() * sizeof(uint32_t));
      for (uint64_t k = 0; k < wn; ++k) X.h_qno.p[k] = Q.number(w0 + k);
      VSX_HIP_AS(WHO, ensure_pinned(X.h_vote, wn));
      if (out->candidates) VSX_HIP_AS(WHO, ensure_pinned(X.h_cand, wn * 2 * SX_ROUNDS));
      VSX_HIP_AS(WHO, X.d_wstart.ensure(nl + 1));
      VSX_HIP_AS(WHO, X.d_qno.ensure(wn));
      VSX_HIP_AS(WHO, X.d_words.ensure(total));
      VSX_HIP_AS(WHO, X.d_samples.ensure(nl * SX_ROUNDS * SX_SUBSET));
      VSX_HIP_AS(WHO, X.d_nsample.ensure(nl * SX_ROUNDS));
      VSX_HIP_AS(WHO, X.d_keys.ensure(nl * SX_ROUNDS * V.ntiles));
      VSX_HIP_AS(WHO, X.d_vote.ensure(wn));
      if (out->candidates) VSX_HIP_AS(WHO, X.d_cand.ensure(wn * 2 * SX_ROUNDS));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_wstart.p, X.h_wstart.p, (nl + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_qno.p, X.h_qno.p, wn * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      if (total) VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_words.p, X.h_words.p, total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      g_stats.seconds_stage += now_s() - t0;

      // ---- sample, count and select, vote
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[0], st));
      VSX_HIP_AS(WHO, vsx_sintax_launch_sample((uint32_t) wn, X.d_wstart.p, X.d_words.p, X.d_qno.p, o.randseed, X.d_samples.p, X.d_nsample.p, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[1], st));
      VSX_HIP_AS(WHO, vsx_sintax_launch_count(V.units, V.bucket_start, V.ntiles, V.nseq, d_len, (uint32_t) nl, X.d_samples.p, X.d_nsample.p,
                                              X.d_keys.p, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[2], st));
      VSX_HIP_AS(WHO, vsx_sintax_launch_vote((uint32_t) wn, V.ntiles, X.d_keys.p, X.d_taxid.p, o.strand_both ? 1 : 0, X.d_vote.p,
                                             out->candidates ? X.d_cand.p : nullptr, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[3], st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_vote.p, X.d_vote.p, wn * sizeof(SxVote), hipMemcpyDeviceToHost, st));
      if (out->candidates) VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_cand.p, X.d_cand.p, wn * 2 * SX_ROUNDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      float ms[3] = {0.f, 0.f, 0.f};
      for (int x = 0; x < 3; ++x) VSX_HIP_AS(WHO, hipEventElapsedTime(&ms[x], X.ev[x], X.ev[x + 1]));
      g_stats.seconds_sample += ms[0] * 1e-3;
      g_stats.seconds_count += ms[1] * 1e-3;
      g_stats.seconds_vote += ms[2] * 1e-3;

      // ---- output
      const double t1 = now_s();
      for (uint64_t k = 0; k < wn; ++k)
        {
          const SxVote & v = X.h_vote.p[k];
          vsx_sintax_record & r = out->rec[w0 + k];
          r.strand = v.strand; r.classified = v.classified;
          for (int s = 0; s < 2; ++s) { r.boot_count[s] = v.boot_count[s]; r.best_count[s] = v.best_count[s]; }
          for (int x = 0; x < SX_RANKS; ++x) { r.rank_seq[x] = v.rank_seq[x]; r.rank_count[x] = v.rank_count[x]; }
        }
      if (out->candidates) std::memcpy(out->candidates + w0 * 2 * SX_ROUNDS, X.h_cand.p, wn * 2 * SX_ROUNDS * sizeof(uint32_t));
      for (uint64_t l = 0; l < nl; ++l) if (lists[l].size() >= SX_SUBSET) { ++g_stats.strands_sampled; g_stats.rounds_counted += SX_ROUNDS; }
      g_stats.tiles = V.ntiles;
      ++g_stats.windows;
      g_stats.seconds_output += now_s() - t1;
    }
  return VSX_OK;
}

int check_call(const vsx_sintax_opts * o, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen,
               vsx_sintax_result * out)
{
  if (!o || !out || (nq && (!qblob || !qoff || !qlen))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (o->randseed == 0) return fail(VSX_EINVAL, "%s: randseed 0 seeds from the operating system: nothing could be compared; give a seed", WHO);
  if (nq > (uint64_t) UINT32_MAX / 2) return fail(VSX_EINVAL, "%s: too many queries in one call", WHO);
  return vsxp::check_spans(WHO, "query", nq, qoff, qlen, qbytes);
}

uint32_t max_dblen()
{
  const uint64_t v = vsxp::env_u64("VSX_SINTAX_MAX_DBLEN", 0);         // tests lower the limit to force the route
  return (v > 0 && v < VSX_SINTAX_MAX_DBLEN) ? (uint32_t) v : VSX_SINTAX_MAX_DBLEN;
}

int run(vsx_searcher * S, const vsx_sintax_opts & o, const Queries & Q, vsx_sintax_result * out)
{
  const uint64_t n = S->len.size();
  if (S->tlabel.size() != n) return fail(VSX_EINVAL, "%s: the database has no labels (vsx_searcher_set_meta): they carry the taxonomy", WHO);
  if (n >= (uint64_t) VSX_SINTAX_NONE) return fail(VSX_EINVAL, "%s: too many database sequences", WHO);
  if (!S->sidx) S->sidx = new VsxSintaxIndex;
  VsxSintaxIndex & X = *S->sidx;
  if (!X.tax_ready)
    {
      const double t0 = now_s();
      std::vector<const char *> lp(n);
      for (uint64_t i = 0; i < n; ++i) lp[i] = S->tlabel[i].c_str();
      X.taxid.assign(n * SX_RANKS, 0);
      intern_labels(n, lp.data(), X.taxid.data(), nullptr, nullptr);
      X.tax_ready = true;
      g_stats.seconds_index += now_s() - t0;
    }
  out->n_queries = Q.n;
  out->rec = (vsx_sintax_record *) std::calloc(std::max<uint64_t>(Q.n, 1), sizeof(vsx_sintax_record));
  if (o.want_candidates) out->candidates = (uint32_t *) std::malloc(std::max<uint64_t>(Q.n, 1) * 2 * SX_ROUNDS * sizeof(uint32_t));
  if (!out->rec || (o.want_candidates && !out->candidates)) return fail(VSX_ENOMEM, "%s: out of memory", WHO);

  // the route of the call
  uint64_t * route = &g_stats.queries_device;
  if (o.sintax_random) route = &g_stats.queries_host_random;
  else if (S->w > 8) route = &g_stats.queries_host_wordlength;
  else if (n && *std::max_element(S->len.begin(), S->len.end()) >= max_dblen()) route = &g_stats.queries_host_dblen;
  else if (!S->ctx || n == 0 || vsxp::env_is_host("VSX_SINTAX")) route = &g_stats.queries_host_forced;
  *route += Q.n;
  if (route == &g_stats.queries_device) { const int rc = run_device(S, X, o, Q, out); if (rc != VSX_OK) return rc; }
  else run_host(S, X, o, Q, out);
  for (uint64_t k = 0; k < Q.n; ++k) out->n_classified += out->rec[k].classified ? 1 : 0;
  return VSX_OK;
}

}  // namespace

void vsx_internal_sintax_index_destroy(VsxSintaxIndex * X)
{
  if (!X) return;
  for (auto & e : X->ev) if (e) (void) hipEventDestroy(e);
  delete X;
}

extern "C" {

void vsx_sintax_opts_default(vsx_sintax_opts * o)
{
  if (!o) return;
  std::memset(o, 0, sizeof *o);
}

void vsx_sintax_result_free(vsx_sintax_result * r)
{
  if (!r) return;
  std::free(r->rec);
  std::free(r->candidates);
  std::memset(r, 0, sizeof *r);
}

void vsx_sintax_last_stats(vsx_sintax_stats * out) { if (out) *out = g_stats; }

int vsx_sintax(vsx_searcher * S, const vsx_sintax_opts * opts, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
               const uint32_t * qlen, uint64_t first_query_no, const uint64_t * query_no, vsx_sintax_result * out)
{
  g_stats = vsx_sintax_stats {};
  const double t_begin = now_s();
  if (!S) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const int rc_q = check_call(opts, nq, qblob, qbytes, qoff, qlen, out);
  if (rc_q != VSX_OK) return rc_q;
  const int rc = run(S, *opts, Queries {nq, qblob, qoff, qlen, first_query_no, query_no}, out);
  if (rc != VSX_OK) { vsx_sintax_result_free(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_sintax_host(const vsx_search_opts * search, const vsx_sintax_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
                             const uint64_t * offsets, const uint32_t * lengths, const char * const * labels, uint64_t nq, const char * qblob,
                             uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen, uint64_t first_query_no, const uint64_t * query_no,
                             vsx_sintax_result * out)
{
  g_stats = vsx_sintax_stats {};
  const double t_begin = now_s();
  if (!search || (n && (!blob || !offsets || !lengths))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const int rc_q = check_call(opts, nq, qblob, qbytes, qoff, qlen, out);
  if (rc_q != VSX_OK) return rc_q;
  if (search->wordlength < 3 || search->wordlength > 15) return fail(VSX_EINVAL, "%s: wordlength must be 3..15", WHO);
  if (search->soft_mask < 0 || search->soft_mask > 2 || search->hardmask < 0 || search->hardmask > 3)
    return fail(VSX_EINVAL, "%s: masking option out of range", WHO);
  if (const int rc = vsxp::check_spans(WHO, "sequence", n, offsets, lengths, blob_bytes)) return rc;
  // a searcher without a context: the masked text, the word length and the labels are all the restatement reads
  vsx_searcher S;
  S.o = *search;
  S.w = (int) search->wordlength;
  S.blob.assign(blob, blob + blob_bytes);
  S.blob.push_back(0);
  S.off.assign(offsets, offsets + n);
  S.len.assign(lengths, lengths + n);
  S.threads = search->threads > 0 ? search->threads : vsxp::usable_cpus();
  if (S.o.soft_mask == 2 && blob_bytes)
    {
      if (!sequences_disjoint(n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (uint64_t) lengths[k]; }))
        return fail(VSX_EINVAL, "%s: DUST masking needs sequences that do not overlap in the blob", WHO);
      dust_states(&S, S.blob.data(), n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (int64_t) lengths[k]; }, (S.o.hardmask & 1) != 0);
    }
  else if (S.o.soft_mask == 1 && (S.o.hardmask & 1) && blob_bytes)
    hardmask_states(&S, S.blob.data(), n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (int64_t) lengths[k]; });
  vsx_seq_meta meta {};
  meta.label = labels;
  int rc = labels ? vsx_searcher_set_meta(&S, &meta) : VSX_OK;
  if (rc == VSX_OK) rc = run(&S, *opts, Queries {nq, qblob, qoff, qlen, first_query_no, query_no}, out);
  vsx_internal_sintax_index_destroy(S.sidx);
  S.sidx = nullptr;
  if (rc != VSX_OK) { vsx_sintax_result_free(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_sintax_intern(uint64_t n, const char * const * labels, uint32_t * ids, int32_t * start, int32_t * len)
{
  if (n && (!labels || !ids)) return fail(VSX_EINVAL, "vsx_internal_sintax_intern: null argument");
  intern_labels(n, labels, ids, start, len);
  return VSX_OK;
}

}  // extern "C"
