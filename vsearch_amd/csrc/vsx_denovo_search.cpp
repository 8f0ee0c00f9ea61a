// vsx_denovo_search.cpp -- de novo chimera detection's part search (vsx_chimera.cpp, vsx_uchime_denovo) on the searcher of vsx_search.cpp.
//
// The reference's de novo loop (core/chimera.cpp:2365-2372) searches query i's 4 parts against an index that holds the non-chimeras
// among 0 .. i-1.  vsx_chimera.cpp runs it in windows of members with speculative passes; this part owns what needs the searcher's
// internals:
//   committed set  the non-chimeras before the window, in a MAIN + DELTA pair of device subset indexes as vsx_cluster_fast keeps its
//                  centroids (a sequence lives in exactly one of them; the union of the two top-N selections holds the top N of the union)
//   window         every part ranked once against the committed set (heap of maxaccepts + maxrejects) and counted against an index of
//                  the window's own members (all members j < the part's query with >= minmatches shared words: the near_device pattern)
//   merge          one part's candidate list for a pass: the heap's top maxaccepts + maxrejects of (committed list U the members
//                  assumed present), in minheap order (count desc, length asc, seqno asc)
//   search         the staged accept / reject replay (run_stages) of a set of parts on their merged lists; the accepted hits of each
//                  part in search_joinhits order (hit_compare_byid)
// Parts the 16-bit tile counters cannot serve (no word of the part, minwordmatches 0, > 32767 words) are counted on the host: with
// minmatches 0 every indexed sequence qualifies (searchcore.cpp:323-337).
#include "vsx_search_internal.h"

using namespace vsxs;

struct VsxDenovo {
  vsx_searcher * S = nullptr;
  struct IxDel { void operator()(VsxKmerIndex * p) const { vsx_kmer_index_destroy(p); } };
  std::unique_ptr<VsxKmerIndex, IxDel> mix, dix, wix;
  std::vector<uint32_t> committed, main_list, delta_list;
  size_t main_n = 0, delta_built = 0;
  KmerAcct kacct;
  uint32_t keep = 20;
  uint64_t s0 = 0, wn = 0;
  std::vector<uint64_t> poff;                       // parts: offsets into the searcher's text
  std::vector<uint32_t> plen, pmember;              // length, window member it belongs to
  std::vector<std::vector<uint32_t>> pwords;
  std::vector<std::vector<Cand>> pc;                // committed candidates, best first, <= keep
  std::vector<std::vector<Cand>> pm;                // window members before the part's query with enough shared words, ascending
  std::vector<std::vector<Cand>> cur;               // the merged lists of the last vsx_internal_denovo_merge per part
  std::vector<uint64_t> seen;
};

static void denovo_host_counts(VsxDenovo & D, uint64_t p, std::vector<uint64_t> & seen)
{
  // a part the device counters do not serve: every committed sequence and every earlier member, counted on the host
  const vsx_searcher & S = *D.S;
  const std::vector<uint32_t> & w = D.pwords[p];
  const uint32_t minmatches = (uint32_t) std::max<int64_t>(0, std::min<int64_t>(S.minwordmatches, (int64_t) w.size()));
  std::vector<uint32_t> tw;
  auto count_of = [&](uint32_t t) -> uint32_t {
    if (w.empty()) return 0;
    unique_kmers(S.blob.data() + S.off[t], S.len[t], S.w, S.o.soft_mask != 0, tw, seen);
    std::sort(tw.begin(), tw.end());
    uint32_t c = 0;
    for (uint32_t k : w) c += std::binary_search(tw.begin(), tw.end(), k) ? 1u : 0u;
    return std::min<uint32_t>(c, 32767);
  };
  std::vector<Cand> & c = D.pc[p];
  c.clear();
  for (uint32_t t : D.committed)
    {
      const uint32_t n = count_of(t);
      if (n >= minmatches) c.push_back(Cand {t, n, S.len[t]});
    }
  const size_t kp = std::min<size_t>(c.size(), D.keep);
  std::partial_sort(c.begin(), c.begin() + (long) kp, c.end(), cand_better);
  c.resize(kp);
  D.pm[p].clear();
  for (uint32_t j = 0; j < D.pmember[p]; ++j)
    {
      const uint32_t t = (uint32_t) (D.s0 + j), n = count_of(t);
      if (n >= minmatches) D.pm[p].push_back(Cand {t, n, S.len[t]});
    }
}

int vsx_internal_denovo_create(vsx_searcher * S, VsxDenovo ** out)
{
  *out = nullptr;
  if (!device_kmer_subsets_ok(*S))
    return fail(VSX_EINVAL, "vsx_uchime_denovo: needs the device k-mer subset indexes: word length 3..8, at least one sequence, VSX_KMER not 'host'");
  std::unique_ptr<VsxDenovo> D(new VsxDenovo);
  D->S = S;
  D->keep = (uint32_t) (S->ma + S->mr);
  VsxKmerIndex * a = nullptr;
  int rc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &a);
  D->mix.reset(a);
  if (rc == VSX_OK) { a = nullptr; rc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &a); D->dix.reset(a); }
  if (rc == VSX_OK) { a = nullptr; rc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &a); D->wix.reset(a); }
  if (rc != VSX_OK) return rc;
  D->seen.assign(seen_words(*S), 0);
  *out = D.release();
  return VSX_OK;
}

void vsx_internal_denovo_destroy(VsxDenovo * D) { delete D; }

int vsx_internal_denovo_window(VsxDenovo * D, uint64_t s0, uint64_t wn, const std::vector<uint64_t> & poff, const std::vector<uint32_t> & plen,
                               const std::vector<uint32_t> & pmember, double * t_rank, double * t_members)
{
  vsx_searcher * S = D->S;
  const double t0 = now_s();
  D->s0 = s0; D->wn = wn;
  D->poff = poff; D->plen = plen; D->pmember = pmember;
  const uint64_t np = poff.size();
  D->pwords.assign(np, {});
  D->pc.assign(np, {});
  D->pm.assign(np, {});
  D->cur.assign(np, {});
  {
    // the parts' unique words, masked as the searcher masks raw queries (lower case left out unless the mode is none)
    const int nth = std::max(1, S->threads);
    std::vector<std::vector<uint64_t>> seen((size_t) nth, std::vector<uint64_t>(D->seen.size(), 0));
    std::atomic<uint64_t> next {0};
    run_pool(nth, [&](int tid) {
      for (;;)
        {
          const uint64_t k = next.fetch_add(64);
          if (k >= np) break;
          for (uint64_t p = k; p < std::min(np, k + 64); ++p)
            unique_kmers(S->blob.data() + poff[p], plen[p], S->w, S->qmode != 0, D->pwords[p], seen[(size_t) tid]);
        }
    });
  }
  // the committed set's indexes catch up with the last commit (main rebuilt when the delta outgrows an eighth of it)
  if (D->committed.size() != D->delta_built)
    {
      const size_t total = D->committed.size();
      int rc;
      if (total - D->main_n > D->main_n / 8 + 2 * wn)
        {
          rc = vsx_kmer_index_rebuild(D->mix.get(), D->committed.data(), total);
          if (rc != VSX_OK) return rc;
          D->main_n = total;
          D->main_list = D->committed;
          D->delta_list.clear();
          static const uint32_t none = 0;                   // (a null list would mean "the whole set")
          rc = vsx_kmer_index_rebuild(D->dix.get(), &none, 0);
        }
      else
        {
          D->delta_list.assign(D->committed.begin() + (long) D->main_n, D->committed.end());
          rc = vsx_kmer_index_rebuild(D->dix.get(), D->delta_list.data(), D->delta_list.size());
        }
      if (rc != VSX_OK) return rc;
      D->delta_built = total;
    }
  std::vector<uint64_t> fallback, ignored;              // (device_rank lists the same parts as `fallback` and leaves them empty)
  for (uint64_t p = 0; p < np; ++p)
    {
      const int64_t mm = std::min<int64_t>(S->minwordmatches, (int64_t) D->pwords[p].size());
      if (mm <= 0 || D->pwords[p].size() > 32767) fallback.push_back(p);
    }
  if (np && !D->main_list.empty())
    {
      const int rc = device_rank(S, D->mix.get(), &D->main_list, np, D->pwords, D->keep, 1024, true, D->pc, ignored, D->kacct);
      if (rc != VSX_OK) return rc;
    }
  if (np && !D->delta_list.empty())
    {
      std::vector<std::vector<Cand>> dc(np);
      const int rc = device_rank(S, D->dix.get(), &D->delta_list, np, D->pwords, D->keep, 1024, true, dc, ignored, D->kacct);
      if (rc != VSX_OK) return rc;
      for (uint64_t p = 0; p < np; ++p)
        {
          if (dc[p].empty()) continue;
          std::vector<Cand> & c = D->pc[p];
          c.insert(c.end(), dc[p].begin(), dc[p].end());
          const size_t kp = std::min<size_t>(c.size(), D->keep);
          std::partial_sort(c.begin(), c.begin() + (long) kp, c.end(), cand_better);
          c.resize(kp);
        }
    }
  const double t1 = now_s();
  *t_rank += t1 - t0;
  // the window's own members: every member j < the part's query with enough shared words (unbounded keep)
  if (np && wn > 1)
    {
      std::vector<uint32_t> wlist(wn);
      for (uint64_t i = 0; i < wn; ++i) wlist[i] = (uint32_t) (s0 + i);
      int rc = vsx_kmer_index_rebuild(D->wix.get(), wlist.data(), wn);
      if (rc != VSX_OK) return rc;
      std::vector<std::vector<Cand>> nc(np);
      rc = device_rank(S, D->wix.get(), &wlist, np, D->pwords, 0xffffffffu, 1024, false, nc, ignored, D->kacct);
      if (rc != VSX_OK) return rc;
      for (uint64_t p = 0; p < np; ++p)
        for (const Cand & c : nc[p])                           // ascending target
          {
            if (c.target >= s0 + pmember[p]) break;            // only earlier members
            D->pm[p].push_back(c);
          }
    }
  for (uint64_t p : fallback) denovo_host_counts(*D, p, D->seen);
  *t_members += now_s() - t1;
  return VSX_OK;
}

// part p's merged candidate list with the window members flagged in present[] (indexed by member): its targets, best first
void vsx_internal_denovo_merge(VsxDenovo * D, uint64_t p, const uint8_t * present, std::vector<uint32_t> & targets)
{
  std::vector<Cand> & c = D->cur[p];
  c = D->pc[p];
  for (const Cand & m : D->pm[p])
    if (present[m.target - D->s0]) c.push_back(m);
  const size_t kp = std::min<size_t>(c.size(), D->keep);
  std::partial_sort(c.begin(), c.begin() + (long) kp, c.end(), cand_better);
  c.resize(kp);
  targets.clear();
  for (const Cand & x : c) targets.push_back(x.target);
}

// the staged search of parts[] on their last merged lists; accepted[k] = part k's accepted targets in search_joinhits order
int vsx_internal_denovo_search(VsxDenovo * D, const std::vector<uint32_t> & parts, std::vector<std::vector<uint32_t>> & accepted,
                               uint64_t * pairs, uint64_t * sentinels)
{
  vsx_searcher * S = D->S;
  const uint64_t np = parts.size();
  accepted.assign(np, {});
  if (!np) return VSX_OK;
  std::string blob;
  std::vector<uint64_t> off(np);
  std::vector<uint32_t> len(np);
  for (uint64_t k = 0; k < np; ++k)
    {
      off[k] = blob.size();
      len[k] = D->plen[parts[k]];
      blob.append(S->blob.data() + D->poff[parts[k]], len[k]);
    }
  vsx_seqset * qset = nullptr;
  int rc = vsx_seqset_create(S->ctx, &qset, np, blob.data(), blob.size(), off.data(), len.data());
  if (rc != VSX_OK) return rc;
  std::vector<QState> st(np);
  for (uint64_t k = 0; k < np; ++k) st[k].cands = D->cur[parts[k]];
  Acct acct;
  auto seq = [&](uint64_t k) { return S->blob.data() + D->poff[parts[k]]; };
  rc = run_stages(*S, st, seq, seq, [&](uint64_t k) { return (int64_t) D->plen[parts[k]]; }, [&](uint64_t k) { return (uint32_t) k; },
                  [&](uint64_t k) { return S->meta_of(D->s0 + D->pmember[parts[k]]); }, qset, acct);
  vsx_seqset_destroy(qset);
  if (rc != VSX_OK) return rc;
  *pairs += acct.pairs;
  *sentinels += acct.sentinels;
  std::vector<Hit *> dst;
  for (uint64_t k = 0; k < np; ++k)
    {
      dst.clear();
      for (Hit & h : st[k].hits) if (h.accepted || h.weak) dst.push_back(&h);
      std::stable_sort(dst.begin(), dst.end(), [](const Hit * a, const Hit * b) { return hit_compare_byid(*a, *b) < 0; });
      for (const Hit * h : dst) if (h->accepted) accepted[k].push_back(h->target);
    }
  return VSX_OK;
}

// the window's non-chimeras join the committed set (Dbindex::add_sequence, chimera.cpp:2365-2372)
void vsx_internal_denovo_commit(VsxDenovo * D, const std::vector<uint32_t> & seqnos)
{
  D->committed.insert(D->committed.end(), seqnos.begin(), seqnos.end());
}
