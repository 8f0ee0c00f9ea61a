// vsx_orient.cpp -- sequence orientation (include/vsx_orient.h), the host side of vsx_orient.hip.
//
// Restated from the reference (src/):
//   orient                         commands/orient.cpp:116-441   the two comparisons per distinct word, the verdict, the text
//   Dbindex::add_sequence          core/dbindex.cpp:121-148      the match count of a word: sequences that contain it
//   unique_count                   core/unique.cpp:155-352       the distinct valid words of a sequence (unique_kmers, vsx_search.cpp)
//
// The first device call builds the match-count table from the searcher's sequence set, chunk by chunk (keys, rocPRIM sort, runs).
// A call then runs its queries in windows: the texts of the window's device queries are packed into one pinned block (the
// caller's offsets may be scattered), the count kernel of each length class writes the records, the emit kernel the oriented text,
// and the host copies both out at the caller's offsets.  Queries the kernels do not serve take the host restatement on the pool.
#include "vsx_search_internal.h"
#include "vsx_orient_internal.h"

using namespace vsxs;
using vsxp::DevBuf;
using vsxp::PinnedBuf;
using vsxp::ensure_pinned;

#define WHO "vsx_orient"

struct VsxOrientIndex {
  // the device table mc[4^w] (w <= 12)
  bool device_ready = false;
  DevBuf<uint32_t> d_mc;
  // the host table: direct for w <= 12, sorted (word, count) pairs beyond
  bool host_ready = false;
  std::vector<uint32_t> h_mc, h_word, h_count;
  // the window's buffers (grow-only, kept between calls)
  PinnedBuf<char> h_text, h_qual, h_otext, h_oqual;
  PinnedBuf<uint64_t> h_off;
  PinnedBuf<uint32_t> h_len, h_list;
  PinnedBuf<OrRec> h_rec;
  DevBuf<char> d_text, d_qual, d_otext, d_oqual;
  DevBuf<uint64_t> d_off;
  DevBuf<uint32_t> d_len, d_list;
  DevBuf<OrRec> d_rec;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

namespace {

thread_local vsx_orient_stats g_stats;

struct Queries { uint64_t n; const char * blob; uint64_t bytes; const uint64_t * off; const uint32_t * len; const char * qual; };

// ---- the host table ----------------------------------------------------------------------------------------------------------
void build_host(const vsx_searcher & S, VsxOrientIndex & X)
{
  if (X.host_ready) return;
  const uint64_t n = S.len.size();
  const int w = S.w;
  const bool soft = S.o.soft_mask != 0;
  const bool direct = w <= VSX_ORIENT_MAX_DEVICE_WORDLENGTH;
  if (direct) X.h_mc.assign((size_t) 1 << (2 * w), 0);
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S.threads), n / 16 + 1));
  std::vector<std::vector<uint32_t>> found((size_t) nth);
  std::atomic<uint64_t> next {0};
  run_pool(nth, [&](int tid) {
    std::vector<uint32_t> words;
    std::vector<uint64_t> seen(seen_words(S), 0);
    for (;;)
      {
        const uint64_t k0 = next.fetch_add(16);
        if (k0 >= n) break;
        for (uint64_t k = k0; k < std::min(n, k0 + 16); ++k)
          {
            unique_kmers(S.blob.data() + S.off[k], (int64_t) S.len[k], w, soft, words, seen);
            if (direct) for (const uint32_t x : words) __atomic_fetch_add(&X.h_mc[x], 1u, __ATOMIC_RELAXED);
            else found[(size_t) tid].insert(found[(size_t) tid].end(), words.begin(), words.end());
          }
      }
  });
  if (!direct)
    {
      std::vector<uint32_t> all;
      for (auto & f : found) { all.insert(all.end(), f.begin(), f.end()); std::vector<uint32_t>().swap(f); }
      std::sort(all.begin(), all.end());
      for (size_t i = 0; i < all.size();)
        {
          size_t j = i;
          while (j < all.size() && all[j] == all[i]) ++j;
          X.h_word.push_back(all[i]);
          X.h_count.push_back((uint32_t) (j - i));
          i = j;
        }
    }
  X.host_ready = true;
}

inline uint32_t host_count(const VsxOrientIndex & X, uint32_t word)
{
  if (!X.h_mc.empty()) return X.h_mc[word];
  const auto it = std::lower_bound(X.h_word.begin(), X.h_word.end(), word);
  return (it != X.h_word.end() && *it == word) ? X.h_count[(size_t) (it - X.h_word.begin())] : 0u;
}

// rc_kmer (commands/orient.cpp:96-113)
inline uint32_t rc_word(uint32_t word, int w)
{
  uint32_t rev = 0;
  for (int i = 0; i < w; ++i) { rev = (rev << 2) | ((word & 3u) ^ 3u); word >>= 2; }
  return rev;
}

inline int32_t verdict(uint32_t nf, uint32_t nr)
{
  if (nf >= 1u && nf >= 4u * nr) return 0;
  if (nr >= 1u && nr >= 4u * nf) return 1;
  return 2;
}

// the oriented text of one query: - reads reverse-complemented / reversed, the others copied
void emit_host(const Queries & Q, uint64_t k, int32_t strand, vsx_orient_result * out)
{
  const uint64_t o = Q.off[k], L = Q.len[k];
  if (strand != 1)
    {
      std::memcpy(out->text + o, Q.blob + o, L);
      if (out->qual) std::memcpy(out->qual + o, Q.qual + o, L);
      return;
    }
  for (uint64_t p = 0; p < L; ++p)
    {
      out->text[o + p] = complement((unsigned char) Q.blob[o + L - 1 - p]);
      if (out->qual) out->qual[o + p] = Q.qual[o + L - 1 - p];
    }
}

// the host restatement over the queries idx[0 .. m) (idx == nullptr: all of Q)
void run_host(const vsx_searcher & S, VsxOrientIndex & X, const vsx_orient_opts & o, const Queries & Q, const uint64_t * idx, uint64_t m,
              vsx_orient_result * out)
{
  if (m == 0) return;
  const double t0 = now_s();
  build_host(S, X);
  g_stats.seconds_build += now_s() - t0;
  const double t1 = now_s();
  const int w = S.w;
  const bool soft = o.qmask != 0;
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) std::max(1, S.threads), m / 8 + 1));
  std::vector<uint64_t> distinct((size_t) nth, 0);
  std::atomic<uint64_t> next {0};
  run_pool(nth, [&](int tid) {
    std::vector<uint32_t> words;
    std::vector<uint64_t> seen(seen_words(S), 0);
    for (;;)
      {
        const uint64_t i0 = next.fetch_add(8);
        if (i0 >= m) break;
        for (uint64_t i = i0; i < std::min(m, i0 + 8); ++i)
          {
            const uint64_t k = idx ? idx[i] : i;
            unique_kmers(Q.blob + Q.off[k], (int64_t) Q.len[k], w, soft, words, seen);
            uint32_t nf = 0, nr = 0;
            for (const uint32_t x : words)
              {
                const uint32_t hf = host_count(X, x), hr = host_count(X, rc_word(x, w));
                if (hf > 8u * hr) ++nf;
                else if (hr > 8u * hf) ++nr;
              }
            distinct[(size_t) tid] += words.size();
            vsx_orient_record & r = out->rec[k];
            r.count_fwd = nf; r.count_rev = nr; r.strand = verdict(nf, nr);
            if (out->text) emit_host(Q, k, r.strand, out);
          }
      }
  });
  for (const uint64_t d : distinct) g_stats.words_distinct += d;
  g_stats.seconds_count += now_s() - t1;
}

// ---- the device table --------------------------------------------------------------------------------------------------------
int build_device(vsx_searcher * S, VsxOrientIndex & X)
{
  if (X.device_ready) return VSX_OK;
  const double t0 = now_s();
  const uint64_t n = S->len.size();
  const int w = S->w;
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
  hipStream_t st = vsx_internal_stream(S->ctx);
  for (auto & e : X.ev) if (!e) VSX_HIP_AS(WHO, hipEventCreate(&e));
  const uint8_t * d_codes; const uint64_t * d_off; const uint32_t * d_len; uint64_t n_all;
  vsx_internal_seqset_device(S->dbset, &d_codes, &d_off, &d_len, &n_all);
  if (n_all != n) return fail(VSX_EHIP, "%s: the searcher's sequence set does not hold its database", WHO);
  const uint8_t * d_lower = vsx_internal_seqset_lower(S->dbset);
  if (S->o.soft_mask != 0 && !d_lower && n) return fail(VSX_EHIP, "%s: a masked database without its case bitmap", WHO);
  const size_t nwords = (size_t) 1 << (2 * w);
  VSX_HIP_AS(WHO, X.d_mc.alloc(nwords));
  VSX_HIP_AS(WHO, hipMemsetAsync(X.d_mc.p, 0, nwords * sizeof(uint32_t), st));

  // chunks of consecutive sequences within the key budget; a sequence longer than the budget is a chunk of its own
  const uint64_t budget_env = vsxp::env_u64("VSX_ORIENT_BUILD_KEYS", 0);             // (tests lower it to cut small databases)
  const uint64_t budget = budget_env ? budget_env : (uint64_t) 1 << 25;               // (here a 0 counts as unset)
  const uint64_t max_seqs = (uint64_t) 1 << 20;
  std::vector<uint64_t> slot_of(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) slot_of[i + 1] = slot_of[i] + S->len[i];
  struct Chunk { uint64_t first, nseq, keys; uint32_t maxlen; };
  std::vector<Chunk> chunks;
  uint64_t max_keys = 0;
  for (uint64_t i = 0; i < n;)
    {
      Chunk c {i, 0, 0, 0};
      while (i < n && c.nseq < max_seqs && (c.nseq == 0 || c.keys + S->len[i] <= budget))
        {
          c.keys += S->len[i];
          c.maxlen = std::max(c.maxlen, S->len[i]);
          ++c.nseq; ++i;
        }
      if (c.keys) chunks.push_back(c);
      max_keys = std::max(max_keys, c.keys);
    }
  DevBuf<uint64_t> d_slot, d_a, d_b;
  DevBuf<char> d_temp;
  VSX_HIP_AS(WHO, d_slot.alloc(n + 1));
  VSX_HIP_AS(WHO, hipMemcpyAsync(d_slot.p, slot_of.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  VSX_HIP_AS(WHO, d_a.alloc(max_keys));
  VSX_HIP_AS(WHO, d_b.alloc(max_keys));
  for (const Chunk & c : chunks)
    {
      unsigned seq_bits = 1;
      while (((uint64_t) 1 << seq_bits) <= c.nseq) ++seq_bits;                    // the sequence field holds 0 .. nseq
      const unsigned end_bit = (unsigned) (2 * w) + seq_bits;
      size_t temp_bytes = 0;
      VSX_HIP_AS(WHO, vsx_orient_sort_keys(nullptr, &temp_bytes, d_a.p, d_b.p, c.keys, end_bit, st));
      VSX_HIP_AS(WHO, d_temp.ensure(temp_bytes));
      VSX_HIP_AS(WHO, vsx_orient_launch_keys(d_codes, d_off, d_len, d_lower, d_slot.p, (uint32_t) c.first, (uint32_t) c.nseq, c.maxlen, w, d_a.p, st));
      VSX_HIP_AS(WHO, vsx_orient_sort_keys(d_temp.p, &temp_bytes, d_a.p, d_b.p, c.keys, end_bit, st));
      VSX_HIP_AS(WHO, vsx_orient_launch_runs(d_b.p, c.keys, (uint32_t) c.nseq, w, X.d_mc.p, st));
      ++g_stats.build_chunks;
      g_stats.build_keys += c.keys;
    }
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  X.device_ready = true;
  g_stats.seconds_build += now_s() - t0;
  return VSX_OK;
}

int class_of(uint32_t len)
{
  for (int c = 0; c < OR_CLASSES; ++c) if (len <= kOrClassQlen[c]) return c;
  return -1;
}

// the device queries of the call, dev[0 .. nd), in windows
int run_device(vsx_searcher * S, VsxOrientIndex & X, const vsx_orient_opts & o, const Queries & Q, const std::vector<uint64_t> & dev,
               vsx_orient_result * out)
{
  const int rc0 = build_device(S, X);
  if (rc0 != VSX_OK) return rc0;
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
  hipStream_t st = vsx_internal_stream(S->ctx);
  const uint64_t window = o.window > 0 ? (uint64_t) o.window : 65536;
  const int hash_bits = (int) vsxp::env_u64("VSX_ORIENT_HASH_BITS", 0);                // tests: long probe chains
  const bool text = out->text != nullptr, qual = out->qual != nullptr;
  const int nth = std::max(1, S->threads);

  for (uint64_t w0 = 0; w0 < dev.size(); w0 += window)
    {
      const uint64_t wn = std::min<uint64_t>(window, dev.size() - w0);
      // ---- stage: the window's texts packed, its queries listed per length class
      const double t0 = now_s();
      VSX_HIP_AS(WHO, ensure_pinned(X.h_off, wn + 1));
      VSX_HIP_AS(WHO, ensure_pinned(X.h_len, wn));
      VSX_HIP_AS(WHO, ensure_pinned(X.h_list, wn));
      VSX_HIP_AS(WHO, ensure_pinned(X.h_rec, wn));
      uint64_t bytes = 0;
      uint64_t per_class[OR_CLASSES] = {0, 0, 0}, class_at[OR_CLASSES + 1];
      for (uint64_t i = 0; i < wn; ++i)
        {
          const uint32_t L = Q.len[dev[w0 + i]];
          X.h_off.p[i] = bytes; X.h_len.p[i] = L;
          bytes += L;
          ++per_class[class_of(L)];
        }
      X.h_off.p[wn] = bytes;
      class_at[0] = 0;
      for (int c = 0; c < OR_CLASSES; ++c) class_at[c + 1] = class_at[c] + per_class[c];
      {
        uint64_t at[OR_CLASSES];
        for (int c = 0; c < OR_CLASSES; ++c) at[c] = class_at[c];
        for (uint64_t i = 0; i < wn; ++i) X.h_list.p[at[class_of(X.h_len.p[i])]++] = (uint32_t) i;
      }
      VSX_HIP_AS(WHO, ensure_pinned(X.h_text, bytes));
      if (qual) VSX_HIP_AS(WHO, ensure_pinned(X.h_qual, bytes));
      if (text) VSX_HIP_AS(WHO, ensure_pinned(X.h_otext, bytes));
      if (qual) VSX_HIP_AS(WHO, ensure_pinned(X.h_oqual, bytes));
      {
        std::atomic<uint64_t> next {0};
        run_pool((int) std::min<uint64_t>((uint64_t) nth, wn / 1024 + 1), [&](int) {
          for (;;)
            {
              const uint64_t i0 = next.fetch_add(1024);
              if (i0 >= wn) break;
              for (uint64_t i = i0; i < std::min(wn, i0 + 1024); ++i)
                {
                  const uint64_t k = dev[w0 + i];
                  std::memcpy(X.h_text.p + X.h_off.p[i], Q.blob + Q.off[k], Q.len[k]);
                  if (qual) std::memcpy(X.h_qual.p + X.h_off.p[i], Q.qual + Q.off[k], Q.len[k]);
                }
            }
        });
      }
      VSX_HIP_AS(WHO, X.d_off.ensure(wn + 1));
      VSX_HIP_AS(WHO, X.d_len.ensure(wn));
      VSX_HIP_AS(WHO, X.d_list.ensure(wn));
      VSX_HIP_AS(WHO, X.d_rec.ensure(wn));
      VSX_HIP_AS(WHO, X.d_text.ensure(bytes));
      if (qual) VSX_HIP_AS(WHO, X.d_qual.ensure(bytes));
      if (text) VSX_HIP_AS(WHO, X.d_otext.ensure(bytes));
      if (qual) VSX_HIP_AS(WHO, X.d_oqual.ensure(bytes));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_off.p, X.h_off.p, (wn + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_len.p, X.h_len.p, wn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_list.p, X.h_list.p, wn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      if (bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_text.p, X.h_text.p, bytes, hipMemcpyHostToDevice, st));
      if (qual && bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(X.d_qual.p, X.h_qual.p, bytes, hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      g_stats.seconds_stage += now_s() - t0;

      // ---- count, emit
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[0], st));
      for (int c = 0; c < OR_CLASSES; ++c)
        VSX_HIP_AS(WHO, vsx_orient_launch_count(c, (uint32_t) per_class[c], X.d_list.p + class_at[c], X.d_text.p, X.d_off.p, X.d_len.p, S->w,
                                                o.qmask != 0 ? 1 : 0, hash_bits, X.d_mc.p, X.d_rec.p, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[1], st));
      if (text)
        VSX_HIP_AS(WHO, vsx_orient_launch_emit((uint32_t) wn, X.d_text.p, qual ? X.d_qual.p : nullptr, X.d_off.p, X.d_len.p, X.d_rec.p,
                                               X.d_otext.p, qual ? X.d_oqual.p : nullptr, st));
      VSX_HIP_AS(WHO, hipEventRecord(X.ev[2], st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      float ms[2] = {0.f, 0.f};
      for (int x = 0; x < 2; ++x) VSX_HIP_AS(WHO, hipEventElapsedTime(&ms[x], X.ev[x], X.ev[x + 1]));
      g_stats.seconds_count += ms[0] * 1e-3;
      g_stats.seconds_emit += ms[1] * 1e-3;

      // ---- output: the records, and the text back at the caller's offsets
      const double t1 = now_s();
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_rec.p, X.d_rec.p, wn * sizeof(OrRec), hipMemcpyDeviceToHost, st));
      if (text && bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_otext.p, X.d_otext.p, bytes, hipMemcpyDeviceToHost, st));
      if (qual && bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(X.h_oqual.p, X.d_oqual.p, bytes, hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      {
        const int nout = (int) std::min<uint64_t>((uint64_t) nth, wn / 1024 + 1);
        std::vector<uint64_t> distinct((size_t) nout, 0);
        std::atomic<uint64_t> next {0};
        run_pool(nout, [&](int tid) {
          for (;;)
            {
              const uint64_t i0 = next.fetch_add(1024);
              if (i0 >= wn) break;
              for (uint64_t i = i0; i < std::min(wn, i0 + 1024); ++i)
                {
                  const uint64_t k = dev[w0 + i];
                  const OrRec & d = X.h_rec.p[i];
                  vsx_orient_record & r = out->rec[k];
                  r.count_fwd = d.count_fwd; r.count_rev = d.count_rev; r.strand = d.strand;
                  distinct[(size_t) tid] += d.distinct;
                  if (text) std::memcpy(out->text + Q.off[k], X.h_otext.p + X.h_off.p[i], Q.len[k]);
                  if (qual) std::memcpy(out->qual + Q.off[k], X.h_oqual.p + X.h_off.p[i], Q.len[k]);
                }
            }
        });
        for (const uint64_t d : distinct) g_stats.words_distinct += d;
      }
      for (int c = 0; c < OR_CLASSES; ++c) g_stats.queries_class[c] += per_class[c];
      ++g_stats.windows;
      g_stats.seconds_output += now_s() - t1;
    }
  return VSX_OK;
}

int check_call(const vsx_orient_opts * o, const Queries & Q, vsx_orient_result * out)
{
  if (!o || !out || (Q.n && (!Q.blob || !Q.off || !Q.len))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (o->qmask < 0 || o->qmask > 2) return fail(VSX_EINVAL, "%s: qmask must be 0 (none), 1 (soft) or 2 (dust)", WHO);
  if (Q.n > (uint64_t) UINT32_MAX) return fail(VSX_EINVAL, "%s: too many queries in one call", WHO);
  if (const int rc = vsxp::check_spans(WHO, "query", Q.n, Q.off, Q.len, Q.bytes)) return rc;
  if (o->want_text && !sequences_disjoint(Q.n, [&](uint64_t k) { return Q.off[k]; }, [&](uint64_t k) { return (uint64_t) Q.len[k]; }))
    return fail(VSX_EINVAL, "%s: want_text needs queries that do not overlap in the blob", WHO);
  return VSX_OK;
}

bool device_serves(const vsx_searcher * S)
{
  return S->ctx && S->dbset && S->w <= VSX_ORIENT_MAX_DEVICE_WORDLENGTH;
}

int run(vsx_searcher * S, const vsx_orient_opts & o, const Queries & Q, vsx_orient_result * out)
{
  if (!S->oidx) S->oidx = new VsxOrientIndex;
  VsxOrientIndex & X = *S->oidx;
  out->n_queries = Q.n;
  out->rec = (vsx_orient_record *) std::calloc(std::max<uint64_t>(Q.n, 1), sizeof(vsx_orient_record));
  if (o.want_text) out->text = (char *) std::calloc(std::max<uint64_t>(Q.bytes, 1), 1);
  if (o.want_text && Q.qual) out->qual = (char *) std::calloc(std::max<uint64_t>(Q.bytes, 1), 1);
  if (!out->rec || (o.want_text && !out->text) || (o.want_text && Q.qual && !out->qual)) return fail(VSX_ENOMEM, "%s: out of memory", WHO);

  // the route of each query
  if (S->w > VSX_ORIENT_MAX_DEVICE_WORDLENGTH || !device_serves(S) || vsxp::env_is_host("VSX_ORIENT"))
    {
      (S->w > VSX_ORIENT_MAX_DEVICE_WORDLENGTH ? g_stats.queries_host_wordlength : g_stats.queries_host_forced) += Q.n;
      run_host(*S, X, o, Q, nullptr, Q.n, out);
    }
  else
    {
      std::vector<uint64_t> dev, host;
      for (uint64_t k = 0; k < Q.n; ++k) (Q.len[k] <= VSX_ORIENT_MAX_QLEN ? dev : host).push_back(k);
      g_stats.queries_device += dev.size();
      g_stats.queries_host_qlen += host.size();
      const int rc = run_device(S, X, o, Q, dev, out);
      if (rc != VSX_OK) return rc;
      run_host(*S, X, o, Q, host.data(), host.size(), out);
    }
  for (uint64_t k = 0; k < Q.n; ++k)
    {
      const int32_t s = out->rec[k].strand;
      if (s == 0) ++out->n_fwd; else if (s == 1) ++out->n_rev; else ++out->n_none;
    }
  return VSX_OK;
}

}  // namespace

void vsx_internal_orient_index_destroy(VsxOrientIndex * X)
{
  if (!X) return;
  for (auto & e : X->ev) if (e) (void) hipEventDestroy(e);
  delete X;
}

extern "C" {

void vsx_orient_opts_default(vsx_orient_opts * o)
{
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->qmask = 2;
}

void vsx_orient_result_free(vsx_orient_result * r)
{
  if (!r) return;
  std::free(r->rec);
  std::free(r->text);
  std::free(r->qual);
  std::memset(r, 0, sizeof *r);
}

void vsx_orient_last_stats(vsx_orient_stats * out) { if (out) *out = g_stats; }

int vsx_orient(vsx_searcher * S, const vsx_orient_opts * opts, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
               const uint32_t * qlen, const char * qualblob, vsx_orient_result * out)
{
  g_stats = vsx_orient_stats {};
  const double t_begin = now_s();
  if (!S) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const Queries Q {nq, qblob, qbytes, qoff, qlen, qualblob};
  const int rc_q = check_call(opts, Q, out);
  if (rc_q != VSX_OK) return rc_q;
  const int rc = run(S, *opts, Q, out);
  if (rc != VSX_OK) { vsx_orient_result_free(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_orient_host(const vsx_search_opts * search, const vsx_orient_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
                             const uint64_t * offsets, const uint32_t * lengths, uint64_t nq, const char * qblob, uint64_t qbytes,
                             const uint64_t * qoff, const uint32_t * qlen, const char * qualblob, vsx_orient_result * out)
{
  g_stats = vsx_orient_stats {};
  const double t_begin = now_s();
  if (!search || (n && (!blob || !offsets || !lengths))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const Queries Q {nq, qblob, qbytes, qoff, qlen, qualblob};
  const int rc_q = check_call(opts, Q, out);
  if (rc_q != VSX_OK) return rc_q;
  if (search->wordlength < 3 || search->wordlength > 15) return fail(VSX_EINVAL, "%s: wordlength must be 3..15", WHO);
  if (search->soft_mask < 0 || search->soft_mask > 2 || search->hardmask < 0 || search->hardmask > 3)
    return fail(VSX_EINVAL, "%s: masking option out of range", WHO);
  if (const int rc = vsxp::check_spans(WHO, "sequence", n, offsets, lengths, blob_bytes)) return rc;
  // a searcher without a context: the masked text and the word length are all the restatement reads
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
  const int rc = run(&S, *opts, Q, out);
  vsx_internal_orient_index_destroy(S.oidx);
  S.oidx = nullptr;
  if (rc != VSX_OK) { vsx_orient_result_free(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_orient_matchcounts(vsx_searcher * S, const uint32_t * words, uint64_t n, uint32_t * counts)
{
  if (!S || (n && (!words || !counts))) return fail(VSX_EINVAL, "vsx_internal_orient_matchcounts: null argument");
  if (!device_serves(S)) return fail(VSX_EINVAL, "vsx_internal_orient_matchcounts: the device route does not serve this searcher");
  if (!S->oidx) S->oidx = new VsxOrientIndex;
  VsxOrientIndex & X = *S->oidx;
  g_stats = vsx_orient_stats {};
  const int rc = build_device(S, X);
  if (rc != VSX_OK) return rc;
  const size_t nwords = (size_t) 1 << (2 * S->w);
  for (uint64_t i = 0; i < n; ++i)
    if (words[i] >= nwords) return fail(VSX_EINVAL, "vsx_internal_orient_matchcounts: word %llu has more than %d bits", (unsigned long long) i, 2 * S->w);
  std::vector<uint32_t> table(nwords);
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(S->ctx)));
  VSX_HIP_AS(WHO, hipMemcpy(table.data(), X.d_mc.p, nwords * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; ++i) counts[i] = table[words[i]];
  return VSX_OK;
}

}  // extern "C"
