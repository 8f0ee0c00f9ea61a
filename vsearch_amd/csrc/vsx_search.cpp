// vsx_search.cpp -- candidate-batch dispatch (include/vsx_search.h): the reference's per-query search loop
// re-expressed as "a window of queries advances in lock step, every stage is one GPU plan".
//
// Restated from the reference (src/, v2.31.0) -- each function cites what it follows:
//   unique k-mers            core/unique.cpp:155-352   (set of valid words; masked/ambiguous symbols poison w words)
//   index                    core/dbindex.cpp:125-255  (k-mer -> targets containing it; list/bitmap split is an
//                                                       implementation detail there, a CSR posting list here)
//   candidate ranking        core/searchcore.cpp:260-340 + core/minheap.cpp:82-146 (count desc, length asc, seqno asc)
//   search loop              core/searchcore.cpp:884-957 ; align_delayed :740-881 ; filters :541-609, :664-737
//   align_trim               core/searchcore.cpp:343-464 ; hit order :133-179, :1028-1052
#include "vsx_search_internal.h"

using namespace vsxs;
using vsxp::usable_cpus;
using vsxp::map4;

namespace vsxs __attribute__((visibility("hidden"))) {

// utils/maps.cpp: chrmap_2bit (:156-186), chrmap_mask_ambig (:208-236), chrmap_mask_lower (:239-267), chrmap_4bit
inline unsigned map2(unsigned char c)
{
  switch (c) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}
inline unsigned mask_ambig(unsigned char c)
{
  switch (c) { case 'A': case 'C': case 'G': case 'T': case 'U': case 'a': case 'c': case 'g': case 't': case 'u': return 0; default: return 1; }
}
inline unsigned mask_lower(unsigned char c)
{
  switch (c) { case 'A': case 'C': case 'G': case 'T': case 'U': return 0; default: return 1; }
}
// seqcmp, utils/seqcmp.cpp:70-92 (4-bit codes, stops at NUL)
static int seqcmp(const char * a, const char * b, int64_t n)
{
  for (int64_t i = 0; i < n; ++i)
    {
      if (a[i] == 0 || b[i] == 0) break;
      const unsigned x = map4((unsigned char) a[i]), y = map4((unsigned char) b[i]);
      if (x < y) return -1;
      if (x > y) return 1;
    }
  return 0;
}

// unique_count, core/unique.cpp:155-352: every distinct word of length w that overlaps no masked symbol.
// `seen` is a 4^w-bit scratch bitmap (w < 10) that is left all-zero on return.
void unique_kmers(const char * seq, int64_t len, int w, bool soft, std::vector<uint32_t> & out, std::vector<uint64_t> & seen)
{
  out.clear();
  const uint64_t mask = (1ull << (2 * w)) - 1;
  uint64_t bad = 0, kmer = 0;
  int64_t s = 0;
  const int64_t e1 = std::min<int64_t>(len, w - 1);
  for (; s < e1; ++s)
    {
      const unsigned char c = (unsigned char) seq[s];
      bad = (bad << 2) | (soft ? mask_lower(c) : mask_ambig(c));
      kmer = (kmer << 2) | map2(c);
    }
  for (; s < len; ++s)
    {
      const unsigned char c = (unsigned char) seq[s];
      bad = ((bad << 2) | (soft ? mask_lower(c) : mask_ambig(c))) & mask;
      kmer = ((kmer << 2) | map2(c)) & mask;
      if (bad == 0)
        {
          if (w < 10)
            {
              uint64_t & word = seen[kmer >> 6];
              const uint64_t bit = 1ull << (kmer & 63);
              if (!(word & bit)) { word |= bit; out.push_back((uint32_t) kmer); }
            }
          else out.push_back((uint32_t) kmer);
        }
    }
  if (w < 10) { for (uint32_t k : out) seen[k >> 6] = 0; }
  else { std::sort(out.begin(), out.end()); out.erase(std::unique(out.begin(), out.end()), out.end()); }
}

// align_trim, core/searchcore.cpp:343-464
void align_trim(Hit & h, int iddef)
{
  h.trim_aln_left = h.trim_q_left = h.trim_t_left = 0;
  h.trim_aln_right = h.trim_q_right = h.trim_t_right = 0;
  const char * const a = h.cigar.c_str();
  const char * p = a;
  if (*p != 0)
    {
      long long run = 1; int scan = 0;
      std::sscanf(p, "%lld%n", &run, &scan);
      const char op = p[scan];
      if (op != 'M')
        {
          h.trim_aln_left = 1 + scan;
          if (op == 'D') h.trim_q_left = (int) run; else h.trim_t_left = (int) run;
        }
    }
  const char * e = a + h.cigar.size();
  if (e > a)
    {
      p = e - 1;
      const char op = *p;
      if (op != 'M')
        {
          while (p > a && *(p - 1) <= '9') --p;
          long long run = 1;
          std::sscanf(p, "%lld", &run);
          h.trim_aln_right = (int) (e - p);
          if (op == 'D') h.trim_q_right = (int) run; else h.trim_t_right = (int) run;
        }
    }
  if (h.trim_q_left >= h.nwalignmentlength) h.trim_q_right = 0;
  if (h.trim_t_left >= h.nwalignmentlength) h.trim_t_right = 0;
  h.internal_alignmentlength = h.nwalignmentlength - h.trim_q_left - h.trim_t_left - h.trim_q_right - h.trim_t_right;
  h.internal_indels = h.nwindels - h.trim_q_left - h.trim_t_left - h.trim_q_right - h.trim_t_right;
  h.internal_gaps = h.nwgaps - ((h.trim_q_left + h.trim_t_left) > 0 ? 1 : 0) - ((h.trim_q_right + h.trim_t_right) > 0 ? 1 : 0);
  h.id0 = h.shortest > 0 ? 100.0 * h.matches / h.shortest : 0.0;
  h.id1 = h.nwalignmentlength > 0 ? 100.0 * h.matches / h.nwalignmentlength : 0.0;
  h.id2 = h.internal_alignmentlength > 0 ? 100.0 * h.matches / h.internal_alignmentlength : 0.0;
  h.id3 = std::max(0.0, 100.0 * (1.0 - (1.0 * (h.mismatches + h.nwgaps) / h.longest)));
  h.id4 = h.nwalignmentlength > 0 ? 100.0 * h.matches / h.nwalignmentlength : 0.0;
  switch (iddef)
    {
    case 0: h.id = h.id0; break;
    case 1: h.id = h.id1; break;
    case 2: h.id = h.id2; break;
    case 3: h.id = h.id3; break;
    case 4: h.id = h.id4; break;
    default: break;
    }
}

// hit_compare_byid_typed, core/searchcore.cpp:133-179 (negative = lhs first)
int hit_compare_byid(const Hit & l, const Hit & r)
{
  if (l.rejected < r.rejected) return -1;
  if (l.rejected > r.rejected) return +1;
  if (l.aligned > r.aligned) return -1;
  if (l.aligned < r.aligned) return +1;
  if (!l.aligned) return 0;
  if (l.id > r.id) return -1;
  if (l.id < r.id) return +1;
  if (l.target < r.target) return -1;
  if (l.target > r.target) return +1;
  return 0;
}

// search_topscores (core/searchcore.cpp:260-340) for one query; counts = zeroed per-thread scratch of size seqcount
void candidates_for(const vsx_searcher & S, const char * q, int64_t qlen, std::vector<uint16_t> & counts,
                    std::vector<uint32_t> & touched, std::vector<uint32_t> & kmers, std::vector<uint64_t> & seen,
                    std::vector<Cand> & out, const IncIndex * inc)
{
  out.clear();
  unique_kmers(q, qlen, S.w, S.qmode != 0, kmers, seen);
  touched.clear();
  auto bump = [&](uint32_t t) {
    uint16_t & c = counts[t];
    if (c == 0) touched.push_back(t);
    if (c < 32767) ++c;                                       // saturates at INT16_MAX (:306-315)
  };
  if (inc) { for (uint32_t k : kmers) for (uint32_t t : inc->post[k]) bump(t); }
  else
    for (uint32_t k : kmers)
      for (uint64_t p = S.kstart[k]; p < S.kstart[k + 1]; ++p) bump(S.postings[p]);
  const uint32_t minmatches = (uint32_t) std::min<int64_t>(S.minwordmatches, (int64_t) kmers.size());   // :320
  if (minmatches == 0)
    {
      // every INDEXED sequence qualifies (the scan runs over dbindex->getcount() entries, :323-337)
      if (inc) { for (uint32_t t = 0; t < S.len.size(); ++t) if (S.is_centroid[t]) out.push_back(Cand {t, counts[t], S.len[t]}); }
      else for (uint32_t t = 0; t < S.len.size(); ++t) out.push_back(Cand {t, counts[t], S.len[t]});
    }
  else
    {
      for (uint32_t t : touched)
        if (counts[t] >= minmatches) out.push_back(Cand {t, counts[t], S.len[t]});
    }
  for (uint32_t t : touched) counts[t] = 0;
  const size_t keep = std::min<size_t>(out.size(), (size_t) S.tophits);       // heap of `tophits` best
  std::partial_sort(out.begin(), out.begin() + keep, out.end(), cand_better);
  out.resize(keep);
}

// Sign of (value - ratio * reference) for two abundances and a size-ratio threshold -- what the abundance filters of
// core/searchcore.cpp:480-537 compare.  Contract (from the reference's behaviour, which callers' outputs depend on):
//   * ratio * reference == 0 (no reference abundance, or a non-positive ratio): positive iff value > 0;
//   * an infinite ratio is larger than any value;
//   * while both abundances are below 2^53 the comparison is the ROUNDED double product ratio * reference against value
//     (long-standing boundary behaviour for ratios like 1/9 must not move);
//   * beyond that it is exact: the double is taken at its stored dyadic value m * 2^e and compared in integers.
// The exact branch here reads m and e from the IEEE-754 fields and decides by magnitude before it shifts anything.
static int abundance_ratio_cmp(int64_t value, double ratio, int64_t reference)
{
  const auto sign_of = [](auto lhs, auto rhs) { return lhs < rhs ? -1 : (rhs < lhs ? 1 : 0); };
  if (reference <= 0 || ratio <= 0.0) return value > 0 ? 1 : 0;
  if (!std::isfinite(ratio)) return -1;
  constexpr int64_t doubles_are_exact_below = int64_t {1} << 53;
  if (value < doubles_are_exact_below && reference < doubles_are_exact_below)
    return sign_of((double) value, ratio * (double) reference);

  typedef unsigned __int128 wide;
  const auto bit_length = [](wide x) { int n = 0; while (x) { ++n; x >>= 1; } return n; };
  uint64_t bits;
  std::memcpy(&bits, &ratio, sizeof bits);
  const uint64_t fraction = bits & ((uint64_t {1} << 52) - 1);
  const int biased = (int) ((bits >> 52) & 0x7ff);
  // ratio = m * 2^e exactly (a subnormal has no hidden bit and the exponent of the smallest normal)
  const uint64_t m = biased ? (fraction | (uint64_t {1} << 52)) : fraction;
  const int e = (biased ? biased : 1) - 1075;
  const wide have = (wide) (uint64_t) value;
  const wide want = (wide) m * (wide) (uint64_t) reference;          // < 2^117: ratio * reference = want * 2^e
  if (e >= 0)
    {
      if (bit_length(want) + e > 64) return -1;                       // want * 2^e >= 2^64 > any 64-bit value
      return sign_of(have, want << e);
    }
  if (have == 0) return -1;                                           // want > 0
  if (bit_length(have) - e > 120) return 1;                           // value * 2^-e >= 2^119 > want
  return sign_of(have << -e, want);
}

// search_acceptable_unaligned, core/searchcore.cpp:541-609
bool acceptable_unaligned(const vsx_searcher & S, const char * q, int64_t qlen, uint32_t target, const QMeta & qm)
{
  const vsx_search_opts & o = S.o;
  const char * d = S.blob.data() + S.off[target];
  const int64_t dlen = S.len[target];
  const double dl = (double) dlen;
  const int64_t tsize = S.abundance(target);
  return (qm.qsize <= o.maxqsize) && (tsize >= o.mintsize) &&
         (abundance_ratio_cmp(qm.qsize, o.minsizeratio, tsize) >= 0) &&
         (abundance_ratio_cmp(qm.qsize, o.maxsizeratio, tsize) <= 0) &&
         (qlen >= o.minqt * dl) && (qlen <= o.maxqt * dl) &&
         (qlen < dlen ? qlen >= o.minsl * dl : dl >= o.minsl * qlen) &&
         (qlen < dlen ? qlen <= o.maxsl * dl : dl <= o.maxsl * qlen) &&
         ((qlen >= o.idprefix) && (dlen >= o.idprefix) && (seqcmp(q, d, o.idprefix) == 0)) &&
         ((qlen >= o.idsuffix) && (dlen >= o.idsuffix) &&
          (seqcmp(q + qlen - o.idsuffix, d + dlen - o.idsuffix, o.idsuffix) == 0)) &&
         ((o.self == 0) || !qm.label || S.tlabel.empty() || (std::strcmp(qm.label, S.tlabel[target].c_str()) != 0)) &&
         ((o.selfid == 0) || (qlen != dlen) || (seqcmp(q, d, qlen) != 0));
}

// alignment_uses_forbidden_gap, core/searchcore.cpp:621-660: an 'I' run is a query gap, a 'D' run a target gap; the first
// CIGAR op is left-terminal, the last right-terminal, any other interior.  An infinite open penalty forbids the class, an
// infinite extension penalty forbids runs longer than one.
static bool uses_forbidden_gap(const std::string & cigar, uint32_t mask)
{
  const char * p = cigar.c_str();
  bool first = true;
  while (*p)
    {
      long long run = 1; int scan = 0;
      std::sscanf(p, "%lld%n", &run, &scan);
      p += scan;
      const char op = *p++;
      if (op == 'I' || op == 'D')
        {
          const bool right = (*p == 0);
          const int cls = first ? 0 : (right ? 4 : 2);            // left, right, interior -> bit of the query-side open penalty
          const int bit = cls + (op == 'I' ? 0 : 1);
          if (mask & (1u << bit)) return true;
          if ((mask & (1u << (6 + bit))) && run > 1) return true;
        }
      first = false;
    }
  return false;
}

// search_acceptable_aligned, core/searchcore.cpp:664-737
bool acceptable_aligned(const vsx_searcher & S, int64_t qlen, Hit & h, int64_t qsize)
{
  const vsx_search_opts & o = S.o;
  if ((h.id >= 100.0 * o.weak_id) && (h.mismatches <= o.maxsubs) && (h.internal_gaps <= o.maxgaps) &&
      ((o.gap_infinite == 0) || !uses_forbidden_gap(h.cigar, o.gap_infinite)) &&
      (h.internal_alignmentlength >= o.mincols) &&
      ((o.leftjust == 0) || (h.trim_q_left + h.trim_t_left == 0)) &&
      ((o.rightjust == 0) || (h.trim_q_right + h.trim_t_right == 0)) &&
      (h.matches + h.mismatches >= o.query_cov * qlen) &&
      (h.matches + h.mismatches >= o.target_cov * (double) S.len[h.target]) &&
      (h.id <= 100.0 * o.maxid) &&
      (100.0 * h.matches / (h.matches + h.mismatches) >= o.mid) &&
      (h.mismatches + h.internal_indels <= o.maxdiffs))
    {
      if (o.cluster_unoise)                                             // UNOISE skew rule (:701-718)
        {
          const double skew = 1.0 * (double) qsize / (double) S.abundance(h.target);
          const double beta = 1.0 / std::pow(2, (1.0 * o.unoise_alpha * h.mismatches) + 1);
          if (skew <= beta || h.mismatches == 0) { h.accepted = true; h.weak = false; return true; }
          h.rejected = true; h.weak = true; return false;
        }
      if (h.id >= 100.0 * o.id) { h.accepted = true; h.weak = false; return true; }
      h.rejected = true; h.weak = true; return false;
    }
  h.rejected = true; h.weak = false;
  return false;
}

// hit_compare_bysize_typed, core/searchcore.cpp:182-243 (negative = lhs first)
int hit_compare_bysize(const vsx_searcher & S, const Hit & l, const Hit & r)
{
  if (l.rejected < r.rejected) return -1;
  if (l.rejected > r.rejected) return +1;
  if (l.rejected) return 0;
  if (l.aligned > r.aligned) return -1;
  if (l.aligned < r.aligned) return +1;
  if (!l.aligned) return 0;
  const int64_t la = S.abundance(l.target), ra = S.abundance(r.target);
  if (la > ra) return -1;
  if (la < ra) return +1;
  if (l.id > r.id) return -1;
  if (l.id < r.id) return +1;
  if (l.target < r.target) return -1;
  if (l.target > r.target) return +1;
  return 0;
}

// The while loop of search_onequery (:915-950) up to the point where align_delayed would be called.
// Returns true if a batch of targets must be aligned now (appended to tq/tt), false if the query is finished.
// LAZY (r05; VERDICT r04 "next" 5): the reference delays 8 candidates, aligns them in one search16 call and then walks them in order
// until maxaccepts or maxrejects is reached -- what lies behind that point was aligned for nothing and is freed unread (:785, :875-878).
// With the default maxaccepts = 1 and a database that holds the query's relatives, that is 7 of the 8 alignments of almost every query.
// A query's FIRST batch here is only as many candidates as it still needs accepts (min(8, maxaccepts)); if they do not finish it, the
// second batch completes the reference's first eight and the batches go on in eights -- the batch boundaries are the reference's from
// there on, so the pairs that reach the aligner are always a SUBSET of the reference's (`pairs_aligned` <= the reference's).  The
// candidates are popped, filtered and judged in the same order under the same two limits, and a hit's verdict does not depend on its
// batch, so accepts, rejects and every reported hit are the reference's.  The sparse-task classes make a window of one-target tasks cheap.
bool advance(const vsx_searcher & S, QState & st, const char * q, int64_t qlen, uint32_t qlocal, const QMeta & qm,
             std::vector<uint32_t> & pq, std::vector<uint32_t> & pt, bool lazy)
{
  const bool first_batch = lazy && st.hits.empty();
  int cap = 8;
  if (first_batch) cap = (int) std::min<int64_t>(8, std::max<int64_t>(1, S.ma));
  else if (lazy && st.lazy_first > 0 && st.lazy_first < 8) { cap = 8 - st.lazy_first; st.lazy_first = 0; }      // back on the reference's boundaries
  while ((st.finalized + st.delayed < S.ma + S.mr - 1) && (st.rejects < S.mr) && (st.accepts < S.ma) &&
         (st.next < st.cands.size()))
    {
      const Cand & c = st.cands[st.next++];            // minheap_poplast: best remaining
      Hit h;
      h.target = c.target; h.count = c.count;
      if (acceptable_unaligned(S, q, qlen, c.target, qm)) ++st.delayed; else h.rejected = true;
      st.hits.push_back(std::move(h));
      if (st.delayed == cap) break;                    // MAXDELAYED (the first batch of a lazy search: what the query still needs)
    }
  if (st.delayed == 0) { st.done = true; return false; }
  if (first_batch) st.lazy_first = st.delayed;
  st.req_first = pq.size();
  st.req_count = 0;
  for (size_t x = (size_t) st.finalized; x < st.hits.size(); ++x)
    if (!st.hits[x].rejected) { pq.push_back(qlocal); pt.push_back(st.hits[x].target); ++st.req_count; }
  return true;
}


// the searcher's acceptance options as the device filter (include/vsx.h): the traceback kernel then decides every pair
// itself and only accepted / weak hits come back with a CIGAR
vsx_filter make_filter(const vsx_searcher & S)
{
  const vsx_search_opts & o = S.o;
  vsx_filter f;
  std::memset(&f, 0, sizeof f);
  f.iddef = o.iddef; f.leftjust = o.leftjust; f.rightjust = o.rightjust;
  f.id = o.id; f.weak_id = o.weak_id; f.maxid = o.maxid; f.mid = o.mid; f.query_cov = o.query_cov; f.target_cov = o.target_cov;
  f.maxsubs = o.maxsubs; f.maxgaps = o.maxgaps; f.mincols = o.mincols; f.maxdiffs = o.maxdiffs;
  return f;
}

void hit_record(const Hit & h, uint32_t q, uint64_t cigar_off, vsx_hit & o)
{
  std::memset(&o, 0, sizeof o);
  o.query = q; o.target = h.target; o.count = h.count;
  o.accepted = h.accepted; o.weak = h.weak; o.used_fallback = h.fallback; o.strand = h.minus ? 1 : 0;
  o.nwscore = h.nwscore; o.nwdiff = h.nwdiff; o.nwgaps = h.nwgaps; o.nwindels = h.nwindels;
  o.nwalignmentlength = h.nwalignmentlength; o.matches = h.matches; o.mismatches = h.mismatches;
  o.internal_alignmentlength = h.internal_alignmentlength; o.internal_gaps = h.internal_gaps;
  o.internal_indels = h.internal_indels;
  o.trim_q_left = h.trim_q_left; o.trim_q_right = h.trim_q_right; o.trim_t_left = h.trim_t_left; o.trim_t_right = h.trim_t_right;
  o.shortest = h.shortest; o.longest = h.longest;
  o.nwid = h.nwid; o.id = h.id; o.id0 = h.id0; o.id1 = h.id1; o.id2 = h.id2; o.id3 = h.id3; o.id4 = h.id4;
  o.cigar_off = cigar_off;
}

int alloc_hits(vsx_hits * out, uint64_t nq, uint64_t n_hits, uint64_t cigar_bytes)
{
  out->n_queries = nq;
  out->n_hits = n_hits;
  out->cigar_bytes = cigar_bytes;
  out->first = (uint64_t *) std::malloc((nq + 1) * sizeof(uint64_t));
  out->hit = (vsx_hit *) std::malloc(std::max<uint64_t>(n_hits, 1) * sizeof(vsx_hit));
  out->cigar_blob = (char *) std::malloc(std::max<uint64_t>(cigar_bytes, 1));
  if (!out->first || !out->hit || !out->cigar_blob) { vsx_hits_free(out); return fail(VSX_ENOMEM, "host allocation failed"); }
  return VSX_OK;
}

int marshal_hits(std::vector<std::vector<Hit>> & kept, vsx_hits * out, int thread_budget)
{
  return marshal_hits_from(kept.size(), [&](uint64_t q) { return HitSpan {kept[q].data(), kept[q].size()}; }, out, thread_budget);
}

// Dbindex::prepare + add_all_sequences (core/dbindex.cpp:163-255): count, prefix-sum, fill
void build_index(vsx_searcher * S)
{
  if (S->indexed) return;
  const uint64_t n = S->len.size();
  const uint64_t nk = 1ull << (2 * S->w);
  S->kstart.assign(nk + 1, 0);
  std::vector<uint64_t> seen(seen_words(*S), 0);
  std::vector<uint32_t> km;
  for (uint64_t i = 0; i < n; ++i)
    {
      unique_kmers(S->blob.data() + S->off[i], S->len[i], S->w, S->o.soft_mask != 0, km, seen);
      for (uint32_t k : km) ++S->kstart[k + 1];
    }
  for (uint64_t k = 0; k < nk; ++k) S->kstart[k + 1] += S->kstart[k];
  S->postings.resize(S->kstart[nk]);
  std::vector<uint64_t> fill(S->kstart.begin(), S->kstart.end() - 1);
  for (uint64_t i = 0; i < n; ++i)
    {
      unique_kmers(S->blob.data() + S->off[i], S->len[i], S->w, S->o.soft_mask != 0, km, seen);
      for (uint32_t k : km) S->postings[fill[k]++] = (uint32_t) i;
    }
  S->indexed = true;
}

// The device path covers every word length the reference accepts (3..15, cli.cc:2934,4198; dbindex.cpp:176-177): 3..8 with one
// bucket per word, 9..15 with tagged postings (vsx_kmer.hip); at least one sequence.  VSX_KMER=host forces the host threads.
bool device_kmer_ok(const vsx_searcher & S)
{
  static const bool forced_host = vsxp::env_is_host("VSX_KMER");
  return !forced_host && S.w >= 3 && S.w <= 15 && !S.len.empty();
}
// clustering rebuilds SUBSET indexes (centroids, round members) every round: those exist for the one-bucket-per-word form only
bool device_kmer_subsets_ok(const vsx_searcher & S) { return device_kmer_ok(S) && S.w <= 8; }

// Count the queries' words against a device index and rank: words[k] = unique words of query k; `map` translates index
// positions to sequence numbers (subset index) or is null; keep = heap size.  cands[k] = (target, count, length) best first
// (rank == true: the heap's total order, cut to `keep`) or all records in position order (rank == false).  Queries the
// 16-bit tile counters cannot serve (threshold 0, > 32767 words) are listed in `fallback` and left empty.
int device_rank(const vsx_searcher * S, VsxKmerIndex * ix, const std::vector<uint32_t> * map, uint64_t nq,
                       const std::vector<std::vector<uint32_t>> & words, uint32_t keep, uint32_t cap_hint, bool rank,
                       std::vector<std::vector<Cand>> & cands, std::vector<uint64_t> & fallback, KmerAcct & acct,
                       int thread_cap)
{
  // CSR + thresholds (:320)
  std::vector<uint64_t> qk_start(nq + 1, 0);
  std::vector<uint32_t> minmatch(nq);
  for (uint64_t k = 0; k < nq; ++k)
    {
      const uint64_t nk = words[k].size();
      const uint64_t mm = (uint64_t) std::min<int64_t>(S->minwordmatches, (int64_t) nk);
      if (mm == 0 || nk > 32767) { minmatch[k] = 0xffffffffu; fallback.push_back(k); qk_start[k + 1] = qk_start[k]; continue; }
      minmatch[k] = (uint32_t) mm;
      qk_start[k + 1] = qk_start[k] + nk;
    }
  std::vector<uint32_t> qk(qk_start[nq]);
  const int nth = std::max(1, thread_cap > 0 ? std::min(thread_cap, S->threads) : S->threads);
  {
    // the words of all queries back to back (threads: a round of clustering is 1.2 M words, a search window 4 M)
    std::atomic<uint64_t> nextq {0};
    auto fill = [&]() {
      for (;;)
        {
          const uint64_t k0 = nextq.fetch_add(256);
          if (k0 >= nq) break;
          for (uint64_t k = k0; k < std::min(nq, k0 + 256); ++k)
            if (minmatch[k] != 0xffffffffu) std::copy(words[k].begin(), words[k].end(), qk.begin() + (int64_t) qk_start[k]);
        }
    };
    const int nfill = (int) std::min<uint64_t>((uint64_t) nth, std::max<uint64_t>(1, nq / 1024));
    run_pool(nfill, [&](int) { fill(); });
  }
  // count on the device; the records come back grouped by query
  VsxKmerResult res;
  VsxKmerStats kst;
  const int rc = vsx_kmer_count_batch(ix, nq, qk_start.data(), qk.data(), minmatch.data(), keep, res, cap_hint, &kst, acct.want_streamed);
  if (rc != VSX_OK) return rc;
  {
    static std::mutex acct_mu;                       // two windows' k-mer stages may finish at once
    std::lock_guard<std::mutex> lk(acct_mu);
    acct.kernel_ms += kst.count_ms;
    acct.streamed += kst.increments;
    acct.streamed_bytes += kst.streamed_bytes;
  }
  // per query: the heap's total order (count desc, length asc, seqno asc) and size
  std::atomic<uint64_t> next {0};
  auto work = [&]() {
    for (;;)
      {
        const uint64_t k = next.fetch_add(1);
        if (k >= nq) break;
        if (minmatch[k] == 0xffffffffu) continue;
        std::vector<Cand> & out = cands[k];
        out.resize(res.cnt[k]);
        for (uint32_t x = 0; x < res.cnt[k]; ++x)
          {
            const uint64_t w = res.rec[res.off[k] + x];
            const uint32_t t = map ? (*map)[(uint32_t) (w & 0xffffffffu)] : (uint32_t) (w & 0xffffffffu);
            out[x] = Cand {t, (uint32_t) (w >> 32), S->len[t]};
          }
        if (rank)
          {
            const size_t kp = std::min<size_t>(out.size(), (size_t) keep);
            std::partial_sort(out.begin(), out.begin() + (int64_t) kp, out.end(), cand_better);
            out.resize(kp);
          }
        else std::sort(out.begin(), out.end(), [](const Cand & a, const Cand & b) { return a.target < b.target; });
      }
  };
  run_pool(nth, [&](int) { work(); });
  return VSX_OK;
}

}  // namespace vsxs

extern "C" {

int vsx_abundance_ratio_cmp(int64_t value, double ratio, int64_t reference) { return abundance_ratio_cmp(value, ratio, reference); }

void vsx_search_opts_default(vsx_search_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->id = -1.0; o->weak_id = 10.0; o->maxaccepts = 1; o->maxrejects = 32; o->wordlength = 8; o->minwordmatches = -1;
  o->iddef = 2; o->soft_mask = 0;
  o->maxsubs = INT_MAX; o->maxgaps = INT_MAX; o->mincols = 0; o->maxdiffs = INT_MAX;
  o->query_cov = 0; o->target_cov = 0; o->maxid = 1.0; o->mid = 0;
  o->minqt = 0; o->maxqt = DBL_MAX; o->minsl = 0; o->maxsl = DBL_MAX;
  o->threads = 0; o->window = 0;
  o->maxqsize = INT64_MAX; o->mintsize = 0; o->minsizeratio = 0.0; o->maxsizeratio = DBL_MAX;
  o->self = 0; o->sizeorder = 0; o->cluster_unoise = 0; o->unoise_alpha = 2.0;
}

int vsx_searcher_create(vsx_ctx * ctx, vsx_searcher ** out, const vsx_search_opts * opts, uint64_t n,
                        const char * blob, uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths)
{
  if (!ctx || !out || !opts || (n && (!blob || !offsets || !lengths))) return fail(VSX_EINVAL, "vsx_searcher_create: null argument");
  *out = nullptr;
  if (opts->id < 0.0 || opts->id > 1.0) return fail(VSX_EINVAL, "vsx_searcher_create: --id must be in [0, 1]");
  if (opts->wordlength < 3 || opts->wordlength > 15) return fail(VSX_EINVAL, "vsx_searcher_create: wordlength must be 3..15");
  if (opts->maxaccepts < 0 || opts->maxrejects < 0) return fail(VSX_EINVAL, "vsx_searcher_create: negative maxaccepts/maxrejects");
  std::unique_ptr<vsx_searcher> S(new vsx_searcher);
  S->ctx = ctx;
  S->scoring = *vsx_internal_scoring(ctx);
  S->o = *opts;
  if (S->o.cluster_unoise) S->o.weak_id = 0.90;                             // cli.cc:4153-4160
  else if (S->o.weak_id > S->o.id) S->o.weak_id = S->o.id;
  S->w = (int) opts->wordlength;
  static const int defaults[16] = {-1, -1, -1, 18, 17, 16, 15, 14, 12, 11, 10, 9, 8, 7, 5, 3};   // searchcore.hpp:75-76
  S->minwordmatches = opts->minwordmatches < 0 ? defaults[S->w] : opts->minwordmatches;
  S->blob.assign(blob, blob + blob_bytes);
  S->blob.push_back(0);
  S->off.assign(offsets, offsets + n);
  S->len.assign(lengths, lengths + n);
  if (const int rc = vsxp::check_spans("vsx_searcher_create", "sequence", n, offsets, lengths, blob_bytes)) return rc;
  // clamp to the database size; 0 means "all" (usearch_global.cpp:598-611)
  const int64_t sc = (int64_t) n;
  S->mr = (opts->maxrejects == 0 || opts->maxrejects > sc) ? sc : opts->maxrejects;
  S->ma = (opts->maxaccepts == 0 || opts->maxaccepts > sc) ? sc : opts->maxaccepts;
  S->tophits = std::min<int64_t>(S->mr + S->ma + 8, sc);
  S->threads = opts->threads > 0 ? opts->threads : usable_cpus();

  // soft masking: the set keeps a case bitmap for its device k-mer index (the alignment itself is case-blind)
  // (2 = DUST: the device masks the set, vsx_mask.hip, and the host copy takes the result over -- from here on a dust-masked
  //  database is a soft-masked one, exactly as in the reference where dust_all rewrites the Database's text, mask.cpp:233-249)
  if (S->o.soft_mask < 0 || S->o.soft_mask > 2) return fail(VSX_EINVAL, "vsx_searcher_create: soft_mask must be 0 (none), 1 (soft) or 2 (dust)");
  if (S->o.qmask < 0 || S->o.qmask > 3) return fail(VSX_EINVAL, "vsx_searcher_create: qmask must be 0 (as soft_mask), 1 (none), 2 (soft) or 3 (dust)");
  S->qmode = S->o.qmask ? S->o.qmask - 1 : S->o.soft_mask;
  if (S->o.soft_mask == 2 && !sequences_disjoint(n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (uint64_t) lengths[k]; }))
    return fail(VSX_EINVAL, "vsx_searcher_create: DUST masking (soft_mask 2) needs sequences that do not overlap in the blob");
  if (S->o.hardmask < 0 || S->o.hardmask > 3) return fail(VSX_EINVAL, "vsx_searcher_create: hardmask must be 0..3 (bit 0: database, bit 1: queries)");
  // r06, --hardmask on the database: the TEXT is rewritten first (host: the option is rare, the exact DUST intervals are needed -- the
  // device bitmap also flags every ambiguity code -- and a symbol that becomes 'N' changes the alignment); what is indexed and aligned
  // from here on is the masked text, with its remaining lower case masked for the k-mers as in every mode but "none"
  const bool hard_db = (S->o.hardmask & 1) && S->o.soft_mask != 0 && blob_bytes;
  if (hard_db)
    {
      if (!sequences_disjoint(n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (uint64_t) lengths[k]; }))
        return fail(VSX_EINVAL, "vsx_searcher_create: --hardmask needs sequences that do not overlap in the blob");
      char * const text = S->blob.data();
      if (S->o.soft_mask == 2) dust_states(S.get(), text, n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (int64_t) lengths[k]; }, true);
      else hardmask_states(S.get(), text, n, [&](uint64_t k) { return offsets[k]; }, [&](uint64_t k) { return (int64_t) lengths[k]; });
      blob = text;
    }
  int rc = S->o.soft_mask ? vsx_internal_seqset_create_cased(ctx, &S->dbset, n, blob, blob_bytes, offsets, lengths, hard_db ? 1 : S->o.soft_mask)
                          : vsx_seqset_create(ctx, &S->dbset, n, blob, blob_bytes, offsets, lengths);
  if (rc != VSX_OK) return rc;
  if (S->o.soft_mask == 2 && blob_bytes && !hard_db)
    {
      std::vector<uint8_t> bits((blob_bytes + 7) / 8);
      rc = vsx_internal_seqset_lower_download(S->dbset, bits.data(), bits.size());
      if (rc != VSX_OK) { vsx_seqset_destroy(S->dbset); return rc; }
      char * const text = S->blob.data();
      const int nth = std::max(1, S->threads);
      const uint64_t step = (blob_bytes + (uint64_t) nth - 1) / (uint64_t) nth;
      auto fold = [&](int t) {
        const uint64_t lo = std::min<uint64_t>(blob_bytes, step * (uint64_t) t), hi = std::min<uint64_t>(blob_bytes, lo + step);
        for (uint64_t i = lo; i < hi; ++i)
          {
            unsigned char c = (unsigned char) text[i];
            if (c >= 'a' && c <= 'z') c = (unsigned char) (c - 32);
            // (a masked ambiguity code stays upper case: it is masked either way, and no k-mer or alignment step reads the case)
            if (((bits[i >> 3] >> (i & 7)) & 1u) && (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'U')) c = (unsigned char) (c | 0x20u);
            text[i] = (char) c;
          }
      };
      run_pool(nth, fold);
    }
  *out = S.release();
  return VSX_OK;
}

int vsx_searcher_set_meta(vsx_searcher * S, const vsx_seq_meta * meta)
{
  if (!S) return fail(VSX_EINVAL, "vsx_searcher_set_meta: null searcher");
  S->tsize.clear();
  S->tlabel.clear();
  vsx_internal_sintax_index_destroy(S->sidx);          // its name ids were cut from the old labels
  S->sidx = nullptr;
  if (!meta) return VSX_OK;
  const uint64_t n = S->len.size();
  if (meta->abundance) S->tsize.assign(meta->abundance, meta->abundance + n);
  if (meta->label)
    {
      S->tlabel.resize(n);
      for (uint64_t i = 0; i < n; ++i) S->tlabel[i] = meta->label[i] ? meta->label[i] : "";
    }
  return VSX_OK;
}

uint64_t vsx_searcher_db_text(const vsx_searcher * s, char * dst, uint64_t cap)
{
  if (!s) return 0;
  const uint64_t n = s->blob.empty() ? 0 : s->blob.size() - 1;          // (the copy carries a terminating NUL)
  if (dst && cap) std::memcpy(dst, s->blob.data(), (size_t) std::min<uint64_t>(cap, n));
  return n;
}

void vsx_searcher_destroy(vsx_searcher * s)
{
  if (!s) return;
  vsx_kmer_index_destroy(s->kidx);
  vsx_internal_exact_index_destroy(s->xidx);
  vsx_internal_sintax_index_destroy(s->sidx);
  vsx_internal_orient_index_destroy(s->oidx);
  vsx_internal_hitout_index_destroy(s->hidx);
  vsx_seqset_destroy(s->dbset);
  vsx_destroy(s->ctx2);
  vsx_destroy(s->ctx3);
  delete s;
}

int64_t vsx_search_candidates(vsx_searcher * S, const char * q, uint32_t qlen, uint32_t * targets, uint32_t * counts, uint64_t cap)
{
  if (!S || (qlen && !q)) return -1;
  build_index(S);
  std::vector<uint16_t> cnt(S->len.size(), 0);
  std::vector<uint32_t> touched, km;
  std::vector<uint64_t> seen(seen_words(*S), 0);
  std::vector<Cand> c;
  std::vector<char> masked, scratch;
  const bool hard_q = (S->o.hardmask & 2) != 0;
  if (S->qmode == 2 && qlen) { masked.assign(q, q + qlen); vsx_internal_dust_one(masked.data(), qlen, scratch, hard_q); q = masked.data(); }
  else if (S->qmode == 1 && hard_q && qlen)
    {
      masked.assign(q, q + qlen);
      for (char & ch : masked) if (((unsigned char) ch & 0x20u) != 0u) ch = 'N';
      q = masked.data();
    }
  candidates_for(*S, q, qlen, cnt, touched, km, seen, c);
  for (size_t i = 0; i < c.size() && i < cap; ++i) { targets[i] = c[i].target; counts[i] = c[i].count; }
  return (int64_t) c.size();
}

int vsx_search_candidates_batch(vsx_searcher * S, int32_t device, uint64_t nq, const char * qblob, uint64_t qbytes,
                                const uint64_t * qoff, const uint32_t * qlen, vsx_candidates * out)
{
  if (!S || !out || (nq && (!qblob || !qoff || !qlen))) return fail(VSX_EINVAL, "vsx_search_candidates_batch: null argument");
  std::memset(out, 0, sizeof *out);
  if (const int rc = vsxp::check_spans("vsx_search_candidates_batch", "query", nq, qoff, qlen, qbytes)) return rc;
  if (device && !device_kmer_ok(*S))
    return fail(VSX_EINVAL, "vsx_search_candidates_batch: the device path needs wordlength 3..15 and a non-empty database");
  const double t0 = now_s();
  std::vector<std::vector<Cand>> cands;
  KmerAcct acct;
  acct.want_streamed = true;                   // this entry reports postings_streamed (bench_kmer.py's roofline)
  std::string masked;
  const bool hard_q = (S->o.hardmask & 2) != 0 && S->qmode != 0;
  if ((S->qmode == 2 || hard_q) && qbytes)
    {
      if (!sequences_disjoint(nq, [&](uint64_t k) { return qoff[k]; }, [&](uint64_t k) { return (uint64_t) qlen[k]; }))
        return fail(VSX_EINVAL, "vsx_search_candidates_batch: DUST / hard query masking needs queries that do not overlap in the blob");
      masked.assign(qblob, qbytes);
      if (S->qmode == 2) dust_states(S, &masked[0], nq, [&](uint64_t k) { return qoff[k]; }, [&](uint64_t k) { return qlen[k]; }, hard_q);
      else hardmask_states(S, &masked[0], nq, [&](uint64_t k) { return qoff[k]; }, [&](uint64_t k) { return qlen[k]; });
      qblob = masked.data();
    }
  const int rc = batch_candidates(S, device != 0, nq, [&](uint64_t k) { return qblob + qoff[k]; },
                                  [&](uint64_t k) { return (int64_t) qlen[k]; }, cands, acct);
  if (rc != VSX_OK) return rc;
  uint64_t total = 0;
  for (auto & c : cands) total += c.size();
  out->n_queries = nq;
  out->start = (uint64_t *) std::malloc((nq + 1) * sizeof(uint64_t));
  out->target = (uint32_t *) std::malloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t));
  out->count = (uint32_t *) std::malloc(std::max<uint64_t>(total, 1) * sizeof(uint32_t));
  if (!out->start || !out->target || !out->count) { vsx_candidates_free(out); return fail(VSX_ENOMEM, "vsx_search_candidates_batch: out of memory"); }
  uint64_t p = 0;
  for (uint64_t k = 0; k < nq; ++k)
    {
      out->start[k] = p;
      for (const Cand & c : cands[k]) { out->target[p] = c.target; out->count[p] = c.count; ++p; }
    }
  out->start[nq] = p;
  out->seconds = now_s() - t0;
  out->kernel_ms = acct.kernel_ms;
  out->index_build_ms = acct.build_ms;
  out->index_postings = acct.postings;
  out->postings_streamed = acct.streamed;
  out->bytes_streamed = acct.streamed_bytes;
  return VSX_OK;
}

void vsx_candidates_free(vsx_candidates * c)
{
  if (!c) return;
  std::free(c->start); std::free(c->target); std::free(c->count);
  std::memset(c, 0, sizeof *c);
}

}  // extern "C"

// ---- vsx_search_batch: windows of queries through three stages (words -> count + rank -> align) ---------------------------------
namespace {

// One window of queries on its way through the stages.  It belongs to whoever holds its unique_ptr -- the words stage makes it, a
// rank worker takes it from the first slot, a consumer from the second -- and nobody else reads or writes it.
struct Window {
  uint64_t w0 = 0, wn = 0, ns = 0, mn = 0, hi = 0;
  std::vector<QState> st;
  std::vector<uint64_t> lo;
  std::vector<uint32_t> ln;
  std::string joined;                            // plus strands + reverse complements as text (only when the host needs them)
  std::vector<std::string> lazy_rc;              // otherwise: single minus strands, built when the fallback aligner asks
  uint64_t rc_off0 = 0;
  const char * wblob = nullptr;
  std::vector<std::vector<uint32_t>> words;      // device k-mer path: unique words per state
  int krc = VSX_OK;
  std::string err;
  double t_kmer = 0;
};

// a window's reported hits, query after query, already in the result's record form (r06: converted by the window's consumer thread -- the
// final marshalling is one pass of block copies; the intermediate Hit objects die with the window, on the thread that made them)
struct WinKept { uint64_t w0 = 0; std::vector<vsx_hit> rec; std::string cigar; std::vector<uint32_t> first; };

// one window in flight between two stages of the piped search
struct Slot {
  std::mutex mu;
  std::condition_variable cv;
  std::unique_ptr<Window> w;
  bool done = false, stop = false;
  bool put(std::unique_ptr<Window> x)       // false: the consumer has given up
  {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return stop || !w; });
    if (stop) return false;
    w = std::move(x);
    cv.notify_all();
    return true;
  }
  std::unique_ptr<Window> get()             // null: the producer has finished
  {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return w || done; });
    std::unique_ptr<Window> x = std::move(w);
    cv.notify_all();
    return x;
  }
  void finish() { std::lock_guard<std::mutex> lk(mu); done = true; cv.notify_all(); }
  void abort() { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); }
};

// Window boundaries of a call of nq queries.  Graded (the piped search at its default window): the first windows are small (the GPU
// starts after the first window's words: a quarter, then half a window), the last two shrink again (half, then a quarter: the last
// alignment stage is the only thing nothing overlaps).  A graded call has more than two windows of queries, so the head and the
// tail always fit and the body takes the rest; every other call is cut into equal windows.
std::vector<uint64_t> window_cuts(uint64_t nq, uint64_t window, bool graded)
{
  std::vector<uint64_t> cut {0};
  const int taper = 2;                                                            // the tail: window / 2, / 4
  uint64_t head_tail = window / 4 + window / 2;
  for (int k = 1; k <= taper; ++k) head_tail += window >> k;
  if (graded && nq > head_tail)
    {
      cut.push_back(window / 4);
      cut.push_back(cut.back() + window / 2);
      const uint64_t body = nq - head_tail;
      for (uint64_t k = 0; k < body / window; ++k) cut.push_back(cut.back() + window);
      if (body % window) cut.push_back(cut.back() + body % window);
      for (int k = 1; k <= taper; ++k) cut.push_back(cut.back() + (window >> k));
    }
  while (cut.back() < nq) cut.push_back(cut.back() + std::min<uint64_t>(std::max<uint64_t>(window, 1), nq - cut.back()));
  return cut;
}

// One call of vsx_search_batch.  The serial form runs every stage of a window on the calling thread; the piped form runs the words
// stage on one thread, up to three rank workers and up to three consumers (the caller is one of them).  Each group of members
// says who may write it.
struct SearchRun {
  // ---- the call and what follows from it: set by the constructor, only read afterwards (any thread) ----
  vsx_searcher * const S;
  const uint64_t nq;
  const char * const qblob;
  const uint64_t * const qoff;
  const uint32_t * const qlen;
  const vsx_seq_meta * const qmeta;
  const bool timeline, lazy_search;
  const double t_begin;
  const std::vector<uint64_t> cut;
  const bool dev_kmer, both;
  const bool dust;                // every strand of every query is DUST-masked on its own (search.cpp:294-303)
  // r06, --hardmask on the queries (search.cpp:294-303): the masked symbols of each strand become 'N' in the text the k-mer stage AND the
  // aligner read -- the window's strands then exist as (masked) text, which is what the device set is made from
  const bool hardq;
  const bool per_strand;          // every strand's words come from its own masked text
  // does any host step read a minus-strand query as text? (host k-mer path; idprefix / idsuffix / selfid compare symbols;
  // the '*' penalties send every pair to the linear-memory aligner)
  const bool need_rc_text;
  // ---- wkept[wi]: written only by the consumer of window wi (consume); marshal reads them after every consumer has been joined ----
  std::vector<WinKept> wkept;
  // ---- the accounting totals: every consumer adds to them, under acc_mu ----
  std::mutex acc_mu;
  double t_align = 0, t_adv = 0, t_rep = 0, t_qset = 0, t_join = 0;
  uint64_t pairs = 0, cells = 0, stages = 0, sentinels = 0;
  // ---- the first error of the piped search and the k-mer time of the windows: the consumers, under rc_mu (serial: the caller) ----
  std::mutex rc_mu;
  int rc = VSX_OK;
  std::string msg;
  double t_kmer = 0;
  // ---- the k-mer stage's statistics: device_rank adds to them under its own mutex ----
  KmerAcct kacct;

  SearchRun(vsx_searcher * S_, uint64_t nq_, const char * qblob_, const uint64_t * qoff_, const uint32_t * qlen_, const vsx_seq_meta * qmeta_,
            bool raw_queries, bool timeline_, bool lazy_, double t_begin_, std::vector<uint64_t> cut_)
    : S(S_), nq(nq_), qblob(qblob_), qoff(qoff_), qlen(qlen_), qmeta(qmeta_), timeline(timeline_), lazy_search(lazy_), t_begin(t_begin_),
      cut(std::move(cut_)), dev_kmer(device_kmer_ok(*S_)), both(S_->o.strand_both != 0), dust(S_->qmode == 2 && !raw_queries),
      hardq((S_->o.hardmask & 2) != 0 && S_->qmode != 0 && !raw_queries), per_strand(dust || hardq),
      need_rc_text(both && (!dev_kmer || S_->o.idprefix > 0 || S_->o.idsuffix > 0 || S_->o.selfid != 0 || S_->o.gap_infinite != 0 || per_strand)),
      wkept(cut.size() - 1)
  {}

  size_t n_windows() const { return cut.size() - 1; }
  size_t window_of(uint64_t w0) const { return (size_t) (std::upper_bound(cut.begin(), cut.end(), w0) - cut.begin()) - 1; }
  void stamp(const char * what, uint64_t w0, double since) const        // VSX_DEBUG_TIMELINE
  {
    std::fprintf(stderr, "  [%7.1f ms] window %llu: %s (%.1f ms)\n", (now_s() - t_begin) * 1e3, (unsigned long long) window_of(w0), what, (now_s() - since) * 1e3);
  }

  // the window's minus strands as text behind the plus strands (W.lo[wn + k] already point there)
  void build_rc_text(Window & W) const
  {
    if (!W.joined.empty()) return;
    const uint64_t span = W.hi - W.mn;
    uint64_t tot = 0;
    for (uint64_t k = 0; k < W.wn; ++k) tot += qlen[W.w0 + k];
    W.joined.assign(qblob + W.mn, span);
    W.joined.resize(span + tot);
    for (uint64_t k = 0; k < W.wn; ++k)
      {
        const char * q = qblob + qoff[W.w0 + k];
        const uint32_t L = qlen[W.w0 + k];
        char * d = &W.joined[W.lo[W.wn + k]];
        for (uint32_t x = 0; x < L; ++x) d[x] = complement((unsigned char) q[L - 1 - x]);
      }
    W.wblob = W.joined.data();
  }

  // stage 1a: the window's sequences (and, on the device k-mer path, their unique words)
  std::unique_ptr<Window> prepare_words(uint64_t w0) const
  {
    std::unique_ptr<Window> W(new Window);
    W->w0 = w0;
    const uint64_t wn = W->wn = cut[window_of(w0) + 1] - w0;
    // --strand both: state k < wn searches query w0 + k, state wn + k its reverse complement (search.cpp:200-214)
    const uint64_t ns = W->ns = both ? 2 * wn : wn;
    W->st.resize(ns);
    // the window's sequences in one blob: the queries, then (both strands) their reverse complements
    uint64_t mn = qoff[w0], hi = qoff[w0];
    for (uint64_t k = 0; k < wn; ++k) { mn = std::min(mn, qoff[w0 + k]); hi = std::max(hi, qoff[w0 + k] + qlen[w0 + k]); }
    W->mn = mn; W->hi = hi;
    W->lo.resize(ns); W->ln.resize(ns);
    for (uint64_t k = 0; k < wn; ++k) { W->lo[k] = qoff[w0 + k] - mn; W->ln[k] = qlen[w0 + k]; }
    // --strand both.  The minus strands exist as TEXT on the host only where the host needs text: the host k-mer path, the
    // prefix / suffix / self filters, the linear-memory fallback.  The aligner's copy is made on the device from the plus
    // strands' codes (vsx_seqset_create_both_strands) and the minus strand's words are the reverse complements of the plus
    // strand's words, so by default no reverse-complemented string is built at all.
    W->wblob = qblob + mn;
    if (both)
      {
        uint64_t tot = 0;
        for (uint64_t k = 0; k < wn; ++k) { W->lo[wn + k] = (hi - mn) + tot; W->ln[wn + k] = qlen[w0 + k]; tot += qlen[w0 + k]; }
        W->rc_off0 = hi - mn;
        if (need_rc_text) build_rc_text(*W);
      }
    Window * w = W.get();
    const double t0 = now_s();
    if (per_strand)
      {
        // masked copies of the window's strands; from here on the window is a soft-masked one
        if (W->joined.empty()) W->joined.assign(qblob + mn, hi - mn);
        if (dust) dust_states(S, &W->joined[0], ns, [w](uint64_t k) { return w->lo[k]; }, [w](uint64_t k) { return w->ln[k]; }, hardq);
        else hardmask_states(S, &W->joined[0], ns, [w](uint64_t k) { return w->lo[k]; }, [w](uint64_t k) { return w->ln[k]; });
        W->wblob = W->joined.data();
      }
    if (dev_kmer)
      {
        kmer_words(S, per_strand ? ns : wn, [w](uint64_t k) { return w->wblob + w->lo[k]; }, [w](uint64_t k) { return (int64_t) w->ln[k]; }, w->words);
        if (both && !per_strand)
          {
            // unique words of the reverse complement = reverse complements of the unique words (a word over unmasked
            // symbols stays one; unique_count's set semantics, core/unique.cpp:155-352): reverse the 2-bit symbols, complement
            w->words.resize(ns);
            const int wl = S->w;
            for (uint64_t k = 0; k < wn; ++k)
              {
                std::vector<uint32_t> & dst = w->words[wn + k];
                dst.resize(w->words[k].size());
                for (size_t x = 0; x < dst.size(); ++x)
                  {
                    uint32_t v = ~w->words[k][x], r = 0;
                    for (int b = 0; b < wl; ++b) { r = (r << 2) | (v & 3u); v >>= 2; }
                    dst[x] = r;
                  }
              }
            // a query the 16-bit tiles cannot serve -- no words at all or --minwordmatches 0 (every sequence is a candidate,
            // searchcore.cpp:283-288), more than 32 767 words -- goes through the host restatement, which reads TEXT: the
            // minus strands must exist as text then (found by oracle/soak_search.py: they were read from unbuilt storage)
            if (W->joined.empty())
              for (uint64_t k = 0; k < wn; ++k)
                {
                  const uint64_t nk = w->words[k].size();
                  if (std::min<int64_t>(S->minwordmatches, (int64_t) nk) == 0 || nk > 32767) { build_rc_text(*W); break; }
                }
          }
      }
    w->t_kmer = now_s() - t0;
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] window %llu: words done (%.1f ms)\n", (now_s() - t_begin) * 1e3, (unsigned long long) window_of(w0), w->t_kmer * 1e3);
    return W;
  }

  // stage 1b: k-mer heuristic for the whole window: device counters (vsx_kmer.hip) or host threads
  void prepare_rank(Window & Wr)
  {
    Window * w = &Wr;
    const double t0 = now_s();
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] window %llu: rank begins\n", (t0 - t_begin) * 1e3, (unsigned long long) window_of(w->w0));
    std::vector<std::vector<Cand>> cands;
    auto seqf = [w](uint64_t k) { return w->wblob + w->lo[k]; };
    auto lenf = [w](uint64_t k) { return (int64_t) w->ln[k]; };
    w->krc = dev_kmer ? kmer_rank(S, w->ns, seqf, lenf, w->words, cands, kacct) : batch_candidates(S, false, w->ns, seqf, lenf, cands, kacct);
    if (w->krc != VSX_OK) w->err = vsx_last_error();
    else
      for (uint64_t k = 0; k < w->ns; ++k) w->st[k].cands = std::move(cands[k]);
    std::vector<std::vector<uint32_t>>().swap(w->words);
    w->t_kmer += now_s() - t0;
    if (timeline) stamp("rank done", w->w0, t0);
  }

  // stage 2: align, replay the accept counters, join the hits
  int consume(Window & W, vsx_ctx * ctx)
  {
    const uint64_t w0 = W.w0, wn = W.wn, ns = W.ns;
    const double tc0 = now_s();
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] window %llu: align begins\n", (tc0 - t_begin) * 1e3, (unsigned long long) window_of(w0));
    auto seq_of = [&](uint64_t k) { return W.wblob + W.lo[k]; };
    std::vector<QState> & st = W.st;
    // the window's sequences as a device sequence set
    vsx_seqset * qset = nullptr;
    const double tq = now_s();
    {
      // both strands: the plus strands are uploaded, the minus strands are made on the device
      // (hard-masked queries: the strands as the masked text -- an 'N' is a different symbol for the aligner)
      int rc2 = hardq ? vsx_seqset_create(ctx, &qset, ns, W.wblob, W.joined.size(), W.lo.data(), W.ln.data())
              : both ? vsx_seqset_create_both_strands(ctx, &qset, wn, qblob + W.mn, W.hi - W.mn, W.lo.data(), W.ln.data())
                     : vsx_seqset_create(ctx, &qset, ns, W.wblob, W.hi - W.mn, W.lo.data(), W.ln.data());
      if (rc2 != VSX_OK) return rc2;
    }
    const double dq = now_s() - tq;
    {
      Acct acct;
      auto meta_of = [&](uint64_t k) {                       // both strands of a query share its abundance and label
        const uint64_t qi = w0 + (k < wn ? k : k - wn);
        return QMeta {(qmeta && qmeta->abundance) ? (int64_t) qmeta->abundance[qi] : 1, (qmeta && qmeta->label) ? qmeta->label[qi] : nullptr};
      };
      // a minus-strand query as text, built on demand (one thread works on a query at a time)
      auto text_of = [&](uint64_t k) -> const char * {
        if (k < wn || !W.joined.empty()) return W.wblob + W.lo[k];
        std::string & r = W.lazy_rc[k - wn];
        if (r.empty() && W.ln[k])
          {
            const char * q = qblob + qoff[w0 + (k - wn)];
            const uint32_t L = W.ln[k];
            r.resize(L);
            for (uint32_t x = 0; x < L; ++x) r[x] = complement((unsigned char) q[L - 1 - x]);
          }
        return r.c_str();
      };
      if (both && W.joined.empty()) W.lazy_rc.assign(wn, std::string());
      const int src = run_stages(*S, st, seq_of, text_of, [&](uint64_t k) { return (int64_t) W.ln[k]; },
                                 [&](uint64_t k) { return (uint32_t) k; }, meta_of, qset, acct, ctx, lazy_search);
      {
        std::lock_guard<std::mutex> lk(acc_mu);
        t_qset += dq;
        t_adv += acct.t_advance; t_rep += acct.t_replay;
        t_align += acct.t_align; pairs += acct.pairs; cells += acct.cells; stages += acct.stages; sentinels += acct.sentinels;
      }
      if (src != VSX_OK) { vsx_seqset_destroy(qset); return src; }
    }
    vsx_seqset_destroy(qset);
    // search_joinhits (:1028-1052): accepted | weak of the plus strand, then of the minus strand, ordered by hit_compare_byid
    const double tj = now_s();
    WinKept & K = wkept[window_of(w0)];
    K.w0 = w0;
    K.first.assign(wn + 1, 0);
    K.rec.reserve(wn + wn / 8);
    std::vector<Hit> dst;
    for (uint64_t k = 0; k < wn; ++k)
      {
        dst.clear();
        for (Hit & h : st[k].hits) if (h.accepted || h.weak) dst.push_back(std::move(h));
        if (both)
          for (Hit & h : st[wn + k].hits) if (h.accepted || h.weak) { h.minus = true; dst.push_back(std::move(h)); }
        // STABLE: the comparator ties when both strands hit the same target with the same identity; the reference's qsort is
        // glibc's merge sort, which keeps the plus-strand hit first (found by oracle/soak_search.py)
        if (dst.size() > 1)
          std::stable_sort(dst.begin(), dst.end(), [](const Hit & a, const Hit & b) { return hit_compare_byid(a, b) < 0; });
        for (const Hit & h : dst)
          {
            K.rec.emplace_back();
            hit_record(h, (uint32_t) (w0 + k), K.cigar.size(), K.rec.back());          // (cigar_off: window-relative until the marshalling)
            K.cigar.append(h.cigar.c_str(), h.cigar.size() + 1);
          }
        K.first[k + 1] = (uint32_t) K.rec.size();
      }
    { std::lock_guard<std::mutex> lk(acc_mu); t_join += now_s() - tj; }
    if (timeline) stamp("align done", w0, tc0);
    return VSX_OK;
  }

  // small batches and a fixed opts.window: every stage of every window on the calling thread
  int run_serial()
  {
    for (size_t wi = 0; wi < n_windows(); ++wi)
      {
        std::unique_ptr<Window> W = prepare_words(cut[wi]);
        prepare_rank(*W);
        t_kmer += W->t_kmer;
        if (W->krc != VSX_OK) { vsx_internal_set_error(W->err.c_str()); return W->krc; }
        const int crc = consume(*W, S->ctx);
        if (crc != VSX_OK) return crc;
      }
    return VSX_OK;
  }

  // ---- the thread bodies of the piped search: each is handed the slots it works between ----
  void words_stage(Slot & to)
  {
    for (size_t wi = 0; wi < n_windows(); ++wi)
      if (!to.put(prepare_words(cut[wi]))) break;
    to.finish();
  }
  void rank_stage(Slot & from, Slot & to, std::atomic<int> & live)
  {
    for (;;)
      {
        std::unique_ptr<Window> W = from.get();
        if (!W) break;
        prepare_rank(*W);
        const bool failed = W->krc != VSX_OK;
        if (!to.put(std::move(W)) || failed) break;
      }
    from.abort();
    if (live.fetch_sub(1) == 1) to.finish();
  }
  void consume_stage(Slot & from, vsx_ctx * ctx)
  {
    for (;;)
      {
        std::unique_ptr<Window> W = from.get();
        if (!W) break;
        int crc = W->krc;
        std::string cmsg = W->err;
        if (crc == VSX_OK)
          {
            crc = consume(*W, ctx);
            if (crc != VSX_OK) cmsg = vsx_last_error();
          }
        std::lock_guard<std::mutex> lk(rc_mu);
        t_kmer += W->t_kmer;
        if (crc != VSX_OK) { if (rc == VSX_OK) { rc = crc; msg = cmsg; } break; }
      }
    from.abort();
  }

  // three stages, one window in flight between each pair: words (host threads) -> count + rank (device, host threads)
  // -> align (this thread and up to two more)
  int run_piped()
  {
    Slot s1, s2;
    std::thread stage_words(&SearchRun::words_stage, this, std::ref(s1));
    // three rank workers on the device k-mer path: one window's host work (CSR, uploads, record download, ranking) runs under another's counting
    // kernel (vsx_kmer_count_batch leases a scratch set and a stream per call); windows may reach the aligner out of order,
    // a query's hits do not depend on it
    const int n_rank = dev_kmer ? 3 : 1;
    std::atomic<int> rank_live {n_rank};
    std::vector<std::thread> stage_rank;
    for (int k = 0; k < n_rank; ++k) stage_rank.emplace_back(&SearchRun::rank_stage, this, std::ref(s1), std::ref(s2), std::ref(rank_live));
    // two consumers, each with its own aligner context on the device (a window's plans, fetches and replays are a chain of
    // short round trips: ~20 ms of wall time for ~5 ms of kernels, so two windows in flight keep the stage off the critical
    // path).  Windows are independent: a query's hits live in its own slot.
    // (r03: three -- a window's align stage is ~12 ms of latency for ~4 ms of kernels while the counting kernels share the device,
    //  and the last window otherwise waits for one of two busy consumers: 147 -> 142 ms per 100 k queries)
    for (vsx_ctx ** extra : {&S->ctx2, &S->ctx3})
      if (!*extra && vsx_create(extra, &S->scoring, vsx_internal_device(S->ctx)) != VSX_OK)
        *extra = nullptr;                                        // (no further context: carry on with fewer consumers)
    for (vsx_ctx * c : {S->ctx, S->ctx2, S->ctx3})
      if (c) { uint64_t drop[2]; vsx_internal_scratch_requests(c, drop, 1); }      // (requests are counted per call: the levelling below)
    std::thread consumer2, consumer3;
    if (S->ctx2) consumer2 = std::thread(&SearchRun::consume_stage, this, std::ref(s2), S->ctx2);
    if (S->ctx3) consumer3 = std::thread(&SearchRun::consume_stage, this, std::ref(s2), S->ctx3);
    consume_stage(s2, S->ctx);
    if (consumer2.joinable()) consumer2.join();
    if (consumer3.joinable()) consumer3.join();
    s2.abort();
    s1.abort();
    stage_words.join();
    for (std::thread & t : stage_rank) t.join();
    if (rc != VSX_OK) { vsx_internal_set_error(msg.c_str()); return rc; }
    // level the consumers' big scratch blocks: whichever context met the largest window sets the size for all, so none of them
    // allocates gigabytes in the middle of a later, warm call (failure to reserve is not an error: that context grows on demand)
    vsx_ctx * all[3] = {S->ctx, S->ctx2, S->ctx3};
    uint64_t want[4] = {0, 0, 0, 0};
    // (levelled to what THIS call's plans asked for, with the blocks' usual headroom -- not to whatever a context happens to hold)
    for (vsx_ctx * c : all)
      if (c)
        {
          uint64_t asked[2];
          vsx_internal_scratch_requests(c, asked, 1);
          want[0] = std::max(want[0], asked[0]);                       // (the bare requests: a block that served them is big enough;
          want[3] = std::max(want[3], asked[1]);                       //  a block that has to grow gets the usual headroom on top)
        }
    // (r06: a consumer's plans follow one another, and vsx_plan_create gives such plans the context's largest idle block: only
    //  block 0 is ever used here, the other two are no longer levelled -- they would be reserved for nothing)
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] stages joined\n", (now_s() - t_begin) * 1e3);
    for (vsx_ctx * c : all) if (c) (void) vsx_internal_scratch_reserve(c, want);
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] scratch levelled\n", (now_s() - t_begin) * 1e3);
    return VSX_OK;
  }

  // windows in query order: their records and CIGAR text back to back, the offsets rebased
  int marshal(vsx_hits * out)
  {
    const double tm = now_s();
    const size_t nw = n_windows();
    std::vector<uint64_t> hbase(nw + 1, 0), cbase(nw + 1, 0);
    for (size_t wi = 0; wi < nw; ++wi) { hbase[wi + 1] = hbase[wi] + wkept[wi].rec.size(); cbase[wi + 1] = cbase[wi] + wkept[wi].cigar.size(); }
    const int arc = alloc_hits(out, nq, hbase[nw], cbase[nw]);
    if (arc != VSX_OK) return arc;
    std::atomic<size_t> next_w {0};
    run_pool((int) std::max<size_t>(1, std::min<size_t>((size_t) std::min(std::max(1, S->threads), 8), nw)), [&](int) {
      for (;;)
        {
          const size_t wi = next_w.fetch_add(1);
          if (wi >= nw) break;
          const WinKept & K = wkept[wi];
          const uint64_t wn = cut[wi + 1] - cut[wi];
          for (uint64_t k = 0; k < wn; ++k) out->first[cut[wi] + k] = hbase[wi] + K.first[k];
          vsx_hit * dst = out->hit + hbase[wi];
          for (size_t x = 0; x < K.rec.size(); ++x) { dst[x] = K.rec[x]; dst[x].cigar_off += cbase[wi]; }
          if (!K.cigar.empty()) std::memcpy(out->cigar_blob + cbase[wi], K.cigar.data(), K.cigar.size());
        }
    });
    out->first[nq] = out->n_hits;
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] hits marshalled\n", (now_s() - t_begin) * 1e3);
    std::vector<WinKept>().swap(wkept);
    if (timeline) std::fprintf(stderr, "  [%7.1f ms] window hits released\n", (now_s() - t_begin) * 1e3);
    out->pairs_aligned = pairs; out->cells_aligned = cells; out->stages = stages; out->sentinel_pairs = sentinels;
    out->seconds_kmer = t_kmer; out->seconds_align = t_align; out->seconds_total = now_s() - t_begin;
    if (std::getenv("VSX_DEBUG_TIMING"))
      std::fprintf(stderr, "vsx_search_batch: kmer %.3f qset %.3f advance %.3f align %.3f replay %.3f join %.3f marshal %.3f total %.3f s\n",
                   t_kmer, t_qset, t_adv, t_align, t_rep, t_join, now_s() - tm, out->seconds_total);
    return VSX_OK;
  }
};

}  // namespace

// raw_queries: the queries are searched as given -- no DUST, no --hardmask of the query text; only the k-mer stage's lower-case
// masking applies (every mode but none).  That is search_onequery called directly, as chimera detection does for its query parts
// (core/chimera.cpp:2023): the query-side masking of --usearch_global lives in search_query (search.cpp:294-303), which it skips.
static int search_batch_impl(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                             const uint32_t * qlen, const vsx_seq_meta * qmeta, vsx_hits * out, bool raw_queries = false)
{
  if (!S || !out || (nq && (!qblob || !qoff || !qlen))) return fail(VSX_EINVAL, "vsx_search_batch: null argument");
  std::memset(out, 0, sizeof *out);
  if (const int rc = vsxp::check_spans("vsx_search_batch", "query", nq, qoff, qlen, qbytes)) return rc;
  const double t_begin = now_s();
  static const bool timeline = std::getenv("VSX_DEBUG_TIMELINE") != nullptr;
  // lazy first batches (advance()): VSX_SEARCH_LAZY=0 aligns the reference's batches of eight from the start (A/B, tests)
  static const bool lazy_search = !(std::getenv("VSX_SEARCH_LAZY") && std::strcmp(std::getenv("VSX_SEARCH_LAZY"), "0") == 0);
  // Windows of queries; the k-mer stage of window i+1 (host word extraction, device counting, host ranking) runs on a
  // producer thread while this thread aligns window i (a query's hits do not depend on its window).  Large batches use
  // smaller windows so that the two stages overlap; small batches and a fixed opts.window run on this thread alone.
  static const uint64_t env_window = std::getenv("VSX_SEARCH_WINDOW") ? std::strtoull(std::getenv("VSX_SEARCH_WINDOW"), nullptr, 10) : 0;   // tests
  const bool piped = env_window ? nq > env_window : (S->o.window <= 0 && nq > 32768);
  const uint64_t window = env_window ? env_window : (S->o.window > 0 ? (uint64_t) S->o.window : (piped ? 16384 : 65536));
  const bool graded = piped && !env_window && S->o.window <= 0;
  SearchRun run(S, nq, qblob, qoff, qlen, qmeta, raw_queries, timeline, lazy_search, t_begin, window_cuts(nq, window, graded));
  const int rc = piped ? run.run_piped() : run.run_serial();
  return rc != VSX_OK ? rc : run.marshal(out);
}

extern "C" {

int vsx_search_batch(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                     const uint32_t * qlen, vsx_hits * out)
{
  return vsx_search_batch_meta(S, nq, qblob, qbytes, qoff, qlen, nullptr, out);
}

int vsx_search_batch_meta(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                          const uint32_t * qlen, const vsx_seq_meta * qmeta, vsx_hits * out)
{
  const double t0 = now_s();
  const int rc = search_batch_impl(S, nq, qblob, qbytes, qoff, qlen, qmeta, out);
  // (seconds_total is what the caller waits for: it includes the release of the call's host state -- r06: that was 8-11 ms of a 130 ms
  //  call and invisible in the call's own accounting, profiles/r06/r06b_search_timeline.txt)
  if (rc == VSX_OK && out) out->seconds_total = now_s() - t0;
  static const bool timing = std::getenv("VSX_DEBUG_TIMING") != nullptr;
  if (timing) std::fprintf(stderr, "vsx_search_batch: returned after %.3f s\n", now_s() - t0);
  return rc;
}

void vsx_hits_free(vsx_hits * h)
{
  if (!h) return;
  std::free(h->first); std::free(h->hit); std::free(h->cigar_blob);
  std::memset(h, 0, sizeof *h);
}

// what vsx_chimera.cpp reads of a searcher: its context, options (weak_id clamped), unclamped scoring, database set and masked text
vsx_ctx * vsx_internal_searcher_ctx(const vsx_searcher * S) { return S->ctx; }
const vsx_search_opts * vsx_internal_searcher_opts(const vsx_searcher * S) { return &S->o; }
const vsx_scoring * vsx_internal_searcher_scoring(const vsx_searcher * S) { return &S->scoring; }
const vsx_seqset * vsx_internal_searcher_dbset(const vsx_searcher * S) { return S->dbset; }
// chimera detection's part search (vsx_chimera.cpp): the parts searched as given (raw_queries above) with candidate heaps of `tophits`
// entries -- chimera_thread_core sizes them maxaccepts + maxrejects (chimera.cpp:2180-2182), --usearch_global adds MAXDELAYED.  The
// searcher's own heap size is restored before returning: the handle behaves as before for every later call.
int vsx_internal_search_parts(vsx_searcher * S, int64_t tophits, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                              const uint32_t * qlen, vsx_hits * out)
{
  if (!S) return fail(VSX_EINVAL, "vsx_internal_search_parts: null searcher");
  struct Restore { vsx_searcher * S; int64_t v; ~Restore() { S->tophits = v; } } restore {S, S->tophits};
  S->tophits = std::min<int64_t>(tophits, (int64_t) S->len.size());
  return search_batch_impl(S, nq, qblob, qbytes, qoff, qlen, nullptr, out, true);
}
void vsx_internal_searcher_text(const vsx_searcher * S, const char ** blob, const uint64_t ** off, const uint32_t ** len)
{
  *blob = S->blob.data(); *off = S->off.data(); *len = S->len.data();
}

}  // extern "C"

bool vsx_internal_searcher_has_abundances(const vsx_searcher * S) { return !S->tsize.empty(); }
