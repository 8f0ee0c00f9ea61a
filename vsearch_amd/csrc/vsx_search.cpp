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

using vsxp::fail;
using vsxp::now_s;
using vsxp::run_pool;
using vsxp::usable_cpus;
using vsxp::map4;

namespace {

// chrmap_complement, utils/maps.cpp:121-150: IUPAC complement, case kept for the letters that have one, everything else 'N'
inline char complement(unsigned char c)
{
  static const char up[] = "TVGHNNCDNNMNKNNNNYSAABWNRN";    // complement of 'A' .. 'Z'
  if (c >= 'A' && c <= 'Z') return up[c - 'A'];
  if (c >= 'a' && c <= 'z')
    {
      const char u = up[c - 'a'];
      const bool kept = std::strchr("abcdghkmnrstuvwy", (int) c) != nullptr;       // letters whose row entry is lower case
      return kept ? (char) (u | 0x20) : 'N';
    }
  return 'N';
}

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
int seqcmp(const char * a, const char * b, int64_t n)
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

}  // namespace

// the query side of one searchinfo_s (core/searchcore.hpp:131-176) beyond the sequence: abundance, label
struct QMeta { int64_t qsize = 1; const char * label = nullptr; };

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
  std::vector<uint64_t> word_total;  // postings per word (statistics of the device index)
  std::vector<uint8_t> is_centroid;  // clustering: which sequences are in the growing index
  std::vector<uint64_t> tsize;       // Database::getabundance of the targets (empty: all 1)
  std::vector<std::string> tlabel;   // Database::getheader (empty: no labels, --self never fires)
  int64_t abundance(uint64_t seqno) const { return tsize.empty() ? 1 : (int64_t) tsize[seqno]; }
  // a database sequence in the query role (allpairs, clustering: si->qsize = db.getabundance, allpairs_global.cpp:398, cluster.cpp:176)
  QMeta meta_of(uint64_t seqno) const { return QMeta {abundance(seqno), tlabel.empty() ? nullptr : tlabel[seqno].c_str()}; }
};


namespace {

// Growing index used by clustering: only centroids are indexed (Dbindex::add_sequence, core/dbindex.cpp:125-152)
struct IncIndex {
  std::vector<std::vector<uint32_t>> post;      // k-mer -> centroid sequence numbers, ascending
  uint64_t indexed = 0;
};

// search_topscores (core/searchcore.cpp:260-340) for one query; counts = zeroed per-thread scratch of size seqcount
void candidates_for(const vsx_searcher & S, const char * q, int64_t qlen, std::vector<uint16_t> & counts,
                    std::vector<uint32_t> & touched, std::vector<uint32_t> & kmers, std::vector<uint64_t> & seen,
                    std::vector<Cand> & out, const IncIndex * inc = nullptr)
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
int abundance_ratio_cmp(int64_t value, double ratio, int64_t reference)
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
bool acceptable_unaligned(const vsx_searcher & S, const char * q, int64_t qlen, uint32_t target, const QMeta & qm = QMeta {})
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
bool uses_forbidden_gap(const std::string & cigar, uint32_t mask)
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
bool acceptable_aligned(const vsx_searcher & S, int64_t qlen, Hit & h, int64_t qsize = 1)
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

}  // namespace

// the searcher's acceptance options as the device filter (include/vsx.h): the traceback kernel then decides every pair
// itself and only accepted / weak hits come back with a CIGAR
static vsx_filter make_filter(const vsx_searcher & S)
{
  const vsx_search_opts & o = S.o;
  vsx_filter f;
  std::memset(&f, 0, sizeof f);
  f.iddef = o.iddef; f.leftjust = o.leftjust; f.rightjust = o.rightjust;
  f.id = o.id; f.weak_id = o.weak_id; f.maxid = o.maxid; f.mid = o.mid; f.query_cov = o.query_cov; f.target_cov = o.target_cov;
  f.maxsubs = o.maxsubs; f.maxgaps = o.maxgaps; f.mincols = o.mincols; f.maxdiffs = o.maxdiffs;
  return f;
}

// Fill a hit from one alignment result (searchcore.cpp:806-857 == allpairs_global.cpp:447-508): linear-memory
// fallback on the sentinel, derived fields, align_trim.  Returns VSX_OK or an error code.
// (qtext() yields the query as text; it is only called on the sentinel path -- minus-strand queries have no text otherwise)
template <typename FQ>
static int fill_hit(const vsx_searcher & S, FQ qtext, int64_t ql, Hit & h, const vsx_results & res, uint64_t r,
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
static void hit_record(const Hit & h, uint32_t q, uint64_t cigar_off, vsx_hit & o)
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
struct HitSpan { const Hit * p; size_t n; const Hit * begin() const { return p; } const Hit * end() const { return p + n; } size_t size() const { return n; } };
template <typename FRange>
static int marshal_hits_from(uint64_t nq, FRange range_of, vsx_hits * out, int thread_budget /* the searcher's: S->threads */)
{
  out->n_queries = nq;
  out->first = (uint64_t *) std::malloc((nq + 1) * sizeof(uint64_t));
  if (!out->first) { vsx_hits_free(out); return fail(VSX_ENOMEM, "host allocation failed"); }
  // positions first (a serial scan over two numbers per query), then the copies on host threads (r04: the serial form was 4-5 ms of a
  // 140 ms search call of 100 k queries)
  std::vector<uint64_t> blob_at(nq + 1);
  uint64_t total = 0, bytes = 0;
  for (uint64_t q = 0; q < nq; ++q)
    {
      out->first[q] = total;
      blob_at[q] = bytes;
      const HitSpan sp = range_of(q);
      total += sp.size();
      for (const Hit & h : sp) bytes += h.cigar.size() + 1;
    }
  out->first[nq] = total;
  blob_at[nq] = bytes;
  out->n_hits = total;
  out->cigar_bytes = bytes;
  out->hit = (vsx_hit *) std::malloc(std::max<uint64_t>(total, 1) * sizeof(vsx_hit));
  out->cigar_blob = (char *) std::malloc(std::max<uint64_t>(bytes, 1));
  if (!out->hit || !out->cigar_blob) { vsx_hits_free(out); return fail(VSX_ENOMEM, "host allocation failed"); }
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

static int marshal_hits(std::vector<std::vector<Hit>> & kept, vsx_hits * out, int thread_budget)
{
  return marshal_hits_from(kept.size(), [&](uint64_t q) { return HitSpan {kept[q].data(), kept[q].size()}; }, out, thread_budget);
}

struct Acct { double t_align = 0, t_advance = 0, t_replay = 0; uint64_t pairs = 0, cells = 0, stages = 0, sentinels = 0; };

// The staged search of a window: every open query contributes its next align_delayed batch, all batches go to the
// GPU as one plan, then the reference's bookkeeping (:782-878) is replayed per query.  qseq/qlen/qidx map a window
// slot to its sequence, length and index inside `qset`.
// qseq(k): the query for the symbol-comparing filters (only dereferenced when idprefix / idsuffix / selfid are set);
// qtext(k): the query as text for the linear-memory fallback (sentinel pairs only; may build it on demand).
template <typename FSeq, typename FText, typename FLen, typename FIdx, typename FMeta>
static int run_stages(const vsx_searcher & S, std::vector<QState> & st, FSeq qseq, FText qtext, FLen qlen, FIdx qidx, FMeta qmeta,
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

// Dbindex::prepare + add_all_sequences (core/dbindex.cpp:163-255): count, prefix-sum, fill
static void build_index(vsx_searcher * S)
{
  if (S->indexed) return;
  const uint64_t n = S->len.size();
  const uint64_t nk = 1ull << (2 * S->w);
  S->kstart.assign(nk + 1, 0);
  std::vector<uint64_t> seen(S->w < 10 ? (nk + 63) / 64 : 1, 0);
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
static bool device_kmer_ok(const vsx_searcher & S)
{
  static const bool forced_host = std::getenv("VSX_KMER") && std::strcmp(std::getenv("VSX_KMER"), "host") == 0;
  return !forced_host && S.w >= 3 && S.w <= 15 && !S.len.empty();
}
// clustering rebuilds SUBSET indexes (centroids, round members) every round: those exist for the one-bucket-per-word form only
static bool device_kmer_subsets_ok(const vsx_searcher & S) { return device_kmer_ok(S) && S.w <= 8; }

struct KmerAcct { double kernel_ms = 0, build_ms = 0; uint64_t streamed = 0, streamed_bytes = 0, postings = 0; bool want_streamed = false; };      // want_streamed: count the postings a batch streams (a serial pass over its words: benches only)

// Count the queries' words against a device index and rank: words[k] = unique words of query k; `map` translates index
// positions to sequence numbers (subset index) or is null; keep = heap size.  cands[k] = (target, count, length) best first
// (rank == true: the heap's total order, cut to `keep`) or all records in position order (rank == false).  Queries the
// 16-bit tile counters cannot serve (threshold 0, > 32767 words) are listed in `fallback` and left empty.
static int device_rank(const vsx_searcher * S, VsxKmerIndex * ix, const std::vector<uint32_t> * map, uint64_t nq,
                       const std::vector<std::vector<uint32_t>> & words, uint32_t keep, uint32_t cap_hint, bool rank,
                       std::vector<std::vector<Cand>> & cands, std::vector<uint64_t> & fallback, KmerAcct & acct,
                       int thread_cap = 0 /* > 0: the caller runs beside other helpers and owns only this share of S->threads */)
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

// DUST rewrites the text in place (host threads per sequence, atomicOr on the device): sequences that share bytes of the blob would
// race and come out with the union of their masks, unlike the reference's per-sequence dust().  Offsets in ascending order (every
// caller of ours) cost one sweep; anything else is sorted first.
template <typename FOff, typename FLen>
static bool sequences_disjoint(uint64_t n, FOff off, FLen len)
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
static void dust_states(const vsx_searcher * S, char * text, uint64_t n, FOff off, FLen len, bool hard = false)
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
static void hardmask_states(const vsx_searcher * S, char * text, uint64_t n, FOff off, FLen len)
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
static void kmer_words(const vsx_searcher * S, uint64_t nq, FSeq qseq, FLen qlen, std::vector<std::vector<uint32_t>> & words)
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
static int kmer_rank(vsx_searcher * S, uint64_t nq, FSeq qseq, FLen qlen, const std::vector<std::vector<uint32_t>> & words,
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
      const uint64_t nwords = 1ull << (2 * S->w);
      build_index(S);
      std::vector<uint16_t> counts(S->len.size(), 0);
      std::vector<uint32_t> touched, km;
      std::vector<uint64_t> seen(S->w < 10 ? (nwords + 63) / 64 : 1, 0);
      for (uint64_t k : fallback) candidates_for(*S, qseq(k), qlen(k), counts, touched, km, seen, cands[k]);
    }
  return VSX_OK;
}

// search_topscores for a batch: cands[k] = candidate list of query k, best first, <= tophits entries.
template <typename FSeq, typename FLen>
static int batch_candidates(vsx_searcher * S, bool device, uint64_t nq, FSeq qseq, FLen qlen,
                            std::vector<std::vector<Cand>> & cands, KmerAcct & acct)
{
  cands.assign(nq, {});
  const int nth = std::max(1, S->threads);
  const uint64_t nwords = 1ull << (2 * S->w);
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
          sc.seen.assign(S->w < 10 ? (nwords + 63) / 64 : 1, 0);
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
  for (uint64_t i = 0; i < n; ++i)
    if (offsets[i] + lengths[i] > blob_bytes) return fail(VSX_EINVAL, "vsx_searcher_create: sequence exceeds the blob");
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
  std::vector<uint64_t> seen(S->w < 10 ? ((1ull << (2 * S->w)) + 63) / 64 : 1, 0);
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
  for (uint64_t i = 0; i < nq; ++i)
    if (qoff[i] + qlen[i] > qbytes) return fail(VSX_EINVAL, "vsx_search_candidates_batch: query exceeds the blob");
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

int vsx_search_batch(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                     const uint32_t * qlen, vsx_hits * out)
{
  return vsx_search_batch_meta(S, nq, qblob, qbytes, qoff, qlen, nullptr, out);
}

// raw_queries: the queries are searched as given -- no DUST, no --hardmask of the query text; only the k-mer stage's lower-case
// masking applies (every mode but none).  That is search_onequery called directly, as chimera detection does for its query parts
// (core/chimera.cpp:2023): the query-side masking of --usearch_global lives in search_query (search.cpp:294-303), which it skips.
static int search_batch_impl(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                             const uint32_t * qlen, const vsx_seq_meta * qmeta, vsx_hits * out, bool raw_queries = false);
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
static int search_batch_impl(vsx_searcher * S, uint64_t nq, const char * qblob, uint64_t qbytes, const uint64_t * qoff,
                             const uint32_t * qlen, const vsx_seq_meta * qmeta, vsx_hits * out, bool raw_queries)
{
  if (!S || !out || (nq && (!qblob || !qoff || !qlen))) return fail(VSX_EINVAL, "vsx_search_batch: null argument");
  std::memset(out, 0, sizeof *out);
  for (uint64_t i = 0; i < nq; ++i)
    if (qoff[i] + qlen[i] > qbytes) return fail(VSX_EINVAL, "vsx_search_batch: query exceeds the blob");
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
  // window boundaries.  Piped: the first windows are small (the GPU starts after the first window's words: a quarter, then half
  // a window), the last two shrink again (half, then a quarter: the last alignment stage is the only thing nothing overlaps)
  std::vector<uint64_t> cut {0};
  const int taper = 2;                                                            // the tail: window / 2, / 4
  const bool graded = piped && !env_window && S->o.window <= 0;
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
  while (cut.back() < nq)
    {
      const uint64_t left = nq - cut.back();
      uint64_t want = window;
      if (graded)
        {
          if (cut.size() == 1) want = window / 4;
          else if (cut.size() == 2) want = window / 2;
          else if (left <= window / 4) want = left;
          else if (left <= window / 2 + window / 4) want = left - window / 4;
          else if (left <= window + window / 2 + window / 4) want = std::min<uint64_t>(window, left - window / 2 - window / 4);
        }
      cut.push_back(cut.back() + std::min<uint64_t>(std::max<uint64_t>(want, 1), left));
    }
  const size_t n_windows = cut.size() - 1;
  auto window_of = [&](uint64_t w0) -> size_t { return (size_t) (std::upper_bound(cut.begin(), cut.end(), w0) - cut.begin()) - 1; };
  // a window's reported hits, query after query, already in the result's record form (r06: converted by the window's consumer thread -- the
  // final marshalling is one pass of block copies; the intermediate Hit objects die with the window, on the thread that made them)
  struct WinKept { uint64_t w0 = 0; std::vector<vsx_hit> rec; std::string cigar; std::vector<uint32_t> first; };
  std::vector<WinKept> wkept(n_windows);
  double t_kmer = 0, t_align = 0, t_adv = 0, t_rep = 0, t_qset = 0, t_join = 0;
  uint64_t pairs = 0, cells = 0, stages = 0, sentinels = 0;

  const bool dev_kmer = device_kmer_ok(*S);
  KmerAcct kacct;
  const bool both = S->o.strand_both != 0;
  // does any host step read a minus-strand query as text? (host k-mer path; idprefix / idsuffix / selfid compare symbols;
  // the '*' penalties send every pair to the linear-memory aligner)
  const bool dust = S->qmode == 2 && !raw_queries;                // every strand of every query is DUST-masked on its own (search.cpp:294-303)
  // r06, --hardmask on the queries (search.cpp:294-303): the masked symbols of each strand become 'N' in the text the k-mer stage AND the
  // aligner read -- the window's strands then exist as (masked) text, which is what the device set is made from
  const bool hardq = (S->o.hardmask & 2) != 0 && S->qmode != 0 && !raw_queries;
  const bool per_strand = dust || hardq;          // every strand's words come from its own masked text
  const bool need_rc_text = both && (!dev_kmer || S->o.idprefix > 0 || S->o.idsuffix > 0 || S->o.selfid != 0 || S->o.gap_infinite != 0 || per_strand);

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
  // the window's minus strands as text behind the plus strands (W.lo[wn + k] already point there)
  auto build_rc_text = [&](Window & W) {
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
  };
  // stage 1a: the window's sequences (and, on the device k-mer path, their unique words)
  auto prepare_words = [&](uint64_t w0) -> std::unique_ptr<Window> {
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
  };
  // stage 1b: k-mer heuristic for the whole window: device counters (vsx_kmer.hip) or host threads
  auto prepare_rank = [&](Window & Wr) {
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
      if (timeline) std::fprintf(stderr, "  [%7.1f ms] window %llu: rank done (%.1f ms)\n", (now_s() - t_begin) * 1e3, (unsigned long long) window_of(w->w0), (now_s() - t0) * 1e3);
  };
  auto prepare = [&](uint64_t w0) -> std::unique_ptr<Window> {
      std::unique_ptr<Window> W = prepare_words(w0);
      prepare_rank(*W);
      return W;
  };
  // stage 2: align, replay the accept counters, join the hits
  std::mutex acc_mu;                            // two consumers add to the accounting
  auto consume = [&](Window & W, vsx_ctx * ctx) -> int {
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
          const size_t from = 0;
          for (Hit & h : st[k].hits) if (h.accepted || h.weak) dst.push_back(std::move(h));
          if (both)
            for (Hit & h : st[wn + k].hits) if (h.accepted || h.weak) { h.minus = true; dst.push_back(std::move(h)); }
          // STABLE: the comparator ties when both strands hit the same target with the same identity; the reference's qsort is
          // glibc's merge sort, which keeps the plus-strand hit first (found by oracle/soak_search.py)
          if (dst.size() - from > 1)
            std::stable_sort(dst.begin() + (long) from, dst.end(), [](const Hit & a, const Hit & b) { return hit_compare_byid(a, b) < 0; });
          for (const Hit & h : dst)
            {
              K.rec.emplace_back();
              hit_record(h, (uint32_t) (w0 + k), K.cigar.size(), K.rec.back());          // (cigar_off: window-relative until the marshalling)
              K.cigar.append(h.cigar.c_str(), h.cigar.size() + 1);
            }
          K.first[k + 1] = (uint32_t) K.rec.size();
        }
      { std::lock_guard<std::mutex> lk(acc_mu); t_join += now_s() - tj; }
      if (timeline) std::fprintf(stderr, "  [%7.1f ms] window %llu: align done (%.1f ms)\n", (now_s() - t_begin) * 1e3, (unsigned long long) window_of(w0), (now_s() - tc0) * 1e3);
      return VSX_OK;
  };

  if (!piped)
    {
      for (size_t wi = 0; wi < n_windows; ++wi)
        {
          std::unique_ptr<Window> W = prepare(cut[wi]);
          t_kmer += W->t_kmer;
          if (W->krc != VSX_OK) { vsx_internal_set_error(W->err.c_str()); return W->krc; }
          const int crc = consume(*W, S->ctx);
          if (crc != VSX_OK) return crc;
        }
    }
  else
    {
      // three stages, one window in flight between each pair: words (host threads) -> count + rank (device, host threads)
      // -> align (this thread)
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
      Slot s1, s2;
      std::thread stage_words([&]() {
        for (size_t wi = 0; wi < n_windows; ++wi)
          if (!s1.put(prepare_words(cut[wi]))) break;
        s1.finish();
      });
      // three rank workers on the device k-mer path: one window's host work (CSR, uploads, record download, ranking) runs under another's counting
      // kernel (vsx_kmer_count_batch leases a scratch set and a stream per call); windows may reach the aligner out of order,
      // a query's hits do not depend on it
      const int n_rank = dev_kmer ? 3 : 1;
      std::atomic<int> rank_live {n_rank};
      auto rank_worker = [&]() {
        for (;;)
          {
            std::unique_ptr<Window> W = s1.get();
            if (!W) break;
            prepare_rank(*W);
            const bool failed = W->krc != VSX_OK;
            if (!s2.put(std::move(W)) || failed) break;
          }
        s1.abort();
        if (rank_live.fetch_sub(1) == 1) s2.finish();
      };
      std::vector<std::thread> stage_rank;
      for (int k = 0; k < n_rank; ++k) stage_rank.emplace_back(rank_worker);
      // two consumers, each with its own aligner context on the device (a window's plans, fetches and replays are a chain of
      // short round trips: ~20 ms of wall time for ~5 ms of kernels, so two windows in flight keep the stage off the critical
      // path).  Windows are independent: a query's hits live in its own slot.
      // (r03: three -- a window's align stage is ~12 ms of latency for ~4 ms of kernels while the counting kernels share the device,
      //  and the last window otherwise waits for one of two busy consumers: 147 -> 142 ms per 100 k queries)
      for (vsx_ctx ** extra : {&S->ctx2, &S->ctx3})
        if (!*extra && vsx_create(extra, &S->scoring, vsx_internal_device(S->ctx)) != VSX_OK)
          *extra = nullptr;                                        // (no further context: carry on with fewer consumers)
      int rc = VSX_OK;
      std::string msg;
      std::mutex rc_mu;
      auto consumer = [&](vsx_ctx * ctx) {
        for (;;)
          {
            std::unique_ptr<Window> W = s2.get();
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
        s2.abort();
      };
      for (vsx_ctx * c : {S->ctx, S->ctx2, S->ctx3})
        if (c) { uint64_t drop[2]; vsx_internal_scratch_requests(c, drop, 1); }      // (requests are counted per call: the levelling below)
      std::thread consumer2, consumer3;
      if (S->ctx2) consumer2 = std::thread(consumer, S->ctx2);
      if (S->ctx3) consumer3 = std::thread(consumer, S->ctx3);
      consumer(S->ctx);
      if (consumer2.joinable()) consumer2.join();
      if (consumer3.joinable()) consumer3.join();
      s2.abort();
      s1.abort();
      stage_words.join();
      for (std::thread & t : stage_rank) t.join();
      if (rc != VSX_OK) { vsx_internal_set_error(msg.c_str()); return rc; }
      // level the consumers' big scratch blocks: whichever context met the largest window sets the size for all, so none of them
      // allocates gigabytes in the middle of a later, warm call (failure to reserve is not an error: that context grows on demand)
      {
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
      }
    }

  // ---- marshal ----
  const double tm = now_s();
  {
    // windows in query order: their records and CIGAR text back to back, the offsets rebased
    std::vector<uint64_t> hbase(n_windows + 1, 0), cbase(n_windows + 1, 0);
    for (size_t wi = 0; wi < n_windows; ++wi) { hbase[wi + 1] = hbase[wi] + wkept[wi].rec.size(); cbase[wi + 1] = cbase[wi] + wkept[wi].cigar.size(); }
    out->n_queries = nq;
    out->n_hits = hbase[n_windows];
    out->cigar_bytes = cbase[n_windows];
    out->first = (uint64_t *) std::malloc((nq + 1) * sizeof(uint64_t));
    out->hit = (vsx_hit *) std::malloc(std::max<uint64_t>(out->n_hits, 1) * sizeof(vsx_hit));
    out->cigar_blob = (char *) std::malloc(std::max<uint64_t>(out->cigar_bytes, 1));
    if (!out->first || !out->hit || !out->cigar_blob) { vsx_hits_free(out); return fail(VSX_ENOMEM, "host allocation failed"); }
    std::atomic<size_t> next_w {0};
    run_pool((int) std::max<size_t>(1, std::min<size_t>((size_t) std::min(std::max(1, S->threads), 8), n_windows)), [&](int) {
      for (;;)
        {
          const size_t wi = next_w.fetch_add(1);
          if (wi >= n_windows) break;
          const WinKept & K = wkept[wi];
          const uint64_t wn = cut[wi + 1] - cut[wi];
          for (uint64_t k = 0; k < wn; ++k) out->first[cut[wi] + k] = hbase[wi] + K.first[k];
          vsx_hit * dst = out->hit + hbase[wi];
          for (size_t x = 0; x < K.rec.size(); ++x) { dst[x] = K.rec[x]; dst[x].cigar_off += cbase[wi]; }
          if (!K.cigar.empty()) std::memcpy(out->cigar_blob + cbase[wi], K.cigar.data(), K.cigar.size());
        }
    });
    out->first[nq] = out->n_hits;
  }
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

// allpairs_global (commands/allpairs_global.cpp:394-527): queries [first, first+count) of the database, each
// against every LATER sequence that passes the unaligned filters (or all of them with acceptall); one GPU
// plan for the whole block; hits kept if acceptall or accepted; order allpairs_hit_compare (:116-138).
// allpairs in three stages (r05: vsx_allpairs_stream overlaps them across blocks; vsx_allpairs_rows runs them back to back):
//   A  ap_enumerate  the pair list of a block of rows            host threads
//   B  ap_align      DP + traceback + filter + ranking            the searcher's aligner context (one call at a time)
//   C  ap_complete   derived hit fields, order, marshalling       host threads
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

// stage C: the host completes the derived fields of the kept hits, orders them and marshals the block's result
static int ap_complete(vsx_searcher * S, int32_t acceptall, const ApList & L, ApAligned & A, vsx_hits * out, int thread_budget)
{
  const uint64_t count = L.rows.size();
  const uint32_t * rows = L.rows.data();
  const uint32_t * pt = L.pt_buf.get();
  const uint64_t n_list = L.n_list;
  const std::vector<uint64_t> & qfirst = L.qfirst;
  std::memset(out, 0, sizeof *out);
  std::vector<std::vector<Hit>> kept(count);
  uint64_t cells = 0, sentinels = 0;
  for (uint64_t k = 0; k < count; ++k) cells += L.cell_part[k];
  int rc = VSX_OK;
  if (A.ranked)
    {
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
            if (resort)
              std::stable_sort(kept[k].begin(), kept[k].end(), [](const Hit & a, const Hit & b) {
                if (a.id != b.id) return a.id > b.id;
                return a.target < b.target;
              });
          }
      };
      {
        run_pool(nth, work);
      }
      for (int t = 0; t < nth; ++t)
        if (err[(size_t) t] != VSX_OK)
          return fail(err[(size_t) t], err[(size_t) t] == VSX_EHIP ? "vsx_allpairs_rows: device and host accept filters disagree"
                                                                     : "vsx_allpairs_rows: fallback aligner failed");
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
              std::stable_sort(kept[k].begin(), kept[k].end(), [](const Hit & a, const Hit & b) {
                if (a.id != b.id) return a.id > b.id;
                return a.target < b.target;
              });
            }
        }
    }
  else
  {
  vsx_results & res = A.res;
  {
    // per query: complete the accepted hits (derived fields, fallback on the sentinel) and order them -- host threads
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
          std::sort(kept[k].begin(), kept[k].end(), [](const Hit & a, const Hit & b) {
            if (a.id != b.id) return a.id > b.id;
            return a.target < b.target;
          });
        }
    };
    run_pool(nth, work);
    for (int t = 0; t < nth; ++t)
      {
        sentinels += psent[(size_t) t];
        if (err[(size_t) t] != VSX_OK)
          return fail(err[(size_t) t], err[(size_t) t] == VSX_EHIP ? "vsx_allpairs_rows: device and host accept filters disagree"
                                                                     : "vsx_allpairs_rows: fallback aligner failed");
      }
  }
  }
  rc = marshal_hits(kept, out, thread_budget);
  if (rc != VSX_OK) return rc;
  for (uint64_t k = 0; k < out->n_hits; ++k) out->hit[k].query = rows[out->hit[k].query];       // vsx_hit.query = database sequence number
  out->pairs_aligned = n_list; out->cells_aligned = cells; out->stages = 1; out->sentinel_pairs = sentinels;
  out->seconds_align = A.t_align; out->seconds_total = now_s() - L.t_begin;
  return VSX_OK;
}

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

// ---------------------------------------------------------------------------------------------------------
// cluster_fast / cluster_smallmem-style greedy centroid clustering (core/cluster.cpp:877-1031 cluster_core_parallel,
// :601-856 evaluate_extra_hits).  Sequences are processed in the given order (the caller sorts: --cluster_fast =
// length descending, Database::sortbylength core/db.cpp:433-450).  A ROUND of `round` sequences is searched against
// the centroids known at the start of the round (one staged GPU search, as vsx_search_batch); the sequential
// reconciliation then replays the reference's intra-round fix-up: sequences of the same round that became centroids
// are inserted into the hit list by shared k-mers and the accept loop is re-run from the top.  The reference
// proves (and the survey verified) that the result does not depend on the round size, i.e. equals the serial
// algorithm; the (query, new-centroid) alignments the fix-up may need are aligned speculatively in one GPU batch.
// ---------------------------------------------------------------------------------------------------------
static bool enough_kmers(const vsx_searcher & S, uint32_t shared, uint32_t kmersamplecount)     // searchcore.cpp:251-257
{
  return ((int64_t) shared >= S.minwordmatches) || (shared >= kmersamplecount);
}

int vsx_cluster_fast(vsx_searcher * S, uint64_t round, vsx_cluster_out * out)
{
  if (!S || !out) return fail(VSX_EINVAL, "vsx_cluster_fast: null argument");
  std::memset(out, 0, sizeof *out);
  // (never silently: a caller asking for --strand both must not get plus-strand clusters back)
  if (S->o.strand_both) return fail(VSX_EINVAL, "vsx_cluster_fast: clustering with --strand both is not provided");
  if (S->qmode != S->o.soft_mask) return fail(VSX_EINVAL, "vsx_cluster_fast: clustering masks everything by soft_mask; qmask must be 0");
  const double t_begin = now_s();
  const uint64_t n = S->len.size();
  if (round == 0) round = 16384;          // (r03: 4096 before; with the next round's main ranking prefetched, fewer and larger rounds win: 10.4 -> 8.5 s at 2 M sequences)
  const uint64_t nk = 1ull << (2 * S->w);
  // r06: the largest plan of the run is a full round with eight candidates per member: its checkpoint block is reserved now, in one
  // piece -- left to grow with the early rounds' plans (few centroids: few candidates) the context re-allocated multi-GB blocks eight times,
  // 1.1 s of a 6-7 s run (profiles/r06/r06e_cluster_blocks.txt).  Sized for the mean length + 10 % (amplicons), never more than a
  // quarter of the device; a run that outgrows it grows the block as before.
  if (n > 0)
    {
      uint64_t tot = 0;
      for (uint64_t i = 0; i < n; ++i) tot += S->len[i];
      const uint32_t typical = (uint32_t) std::min<uint64_t>(65535, tot / n + tot / n / 10 + 1);
      uint64_t want[4] = {vsx_internal_ckpt_bytes_estimate(S->ctx, std::min<uint64_t>(round, n), typical, typical), 0, 0, 0};
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
      want[0] = std::min<uint64_t>(want[0], (uint64_t) free_b / 4);
      if (want[0] >= (16ull << 20)) (void) vsx_internal_scratch_reserve(S->ctx, want);
    }
  IncIndex inc;
  inc.post.assign(nk, {});
  S->is_centroid.assign(n, 0);
  std::vector<uint32_t> clusterno(n, 0);
  // r06: a member's one reported hit goes straight into the result's record form, in sequence order (a vector of Hit per sequence was
  // 1.2 M small blocks made one by one and released one by one at return)
  std::vector<vsx_hit> kept_rec;
  std::string kept_cigar;
  uint32_t nclusters = 0;
  Acct acct;
  double t_kmer = 0;
  double tm_words = 0, tm_rebuild = 0, tm_rank = 0, tm_stages = 0, tm_near = 0, tm_spec = 0, tm_recon = 0, tm_free = 0;      // VSX_DEBUG_TIMING
  const int64_t hit_capacity = std::min<int64_t>(S->ma + S->mr - 1, S->tophits);

  const int nth = std::max(1, S->threads);
  struct Scratch { std::vector<uint16_t> counts; std::vector<uint32_t> touched, km; std::vector<uint64_t> seen; };
  std::vector<Scratch> scratch((size_t) nth);
  for (auto & sc : scratch)
    {
      sc.counts.assign(n, 0);
      sc.seen.assign(S->w < 10 ? (nk + 63) / 64 : 1, 0);
    }
  auto seq_of = [&](uint64_t seqno) { return S->blob.data() + S->off[seqno]; };

  // device k-mer counting (vsx_kmer.hip): one index over the centroids, rebuilt when a round added some, and one over the
  // members of the current round (the intra-round shared-word counts of evaluate_extra_hits)
  const bool dev_kmer = device_kmer_subsets_ok(*S);
  struct IxDel { void operator()(VsxKmerIndex * p) const { vsx_kmer_index_destroy(p); } };
  // The centroid index grows by up to `round` sequences per round (Dbindex::add_sequence, cluster.cpp:1009).  Rebuilding it
  // every round cost 15 % of a 1 M-sequence run and grows quadratically; instead a MAIN index is rebuilt only when the DELTA
  // index over the centroids added since has grown past an eighth of it, the small delta is rebuilt every round, and a query is
  // counted against both: a centroid lives in exactly one of them, thresholds are per sequence, and the union of the two
  // top-N selections contains the top N of the union.
  std::unique_ptr<VsxKmerIndex, IxDel> cix, dix, rix;
  std::vector<uint32_t> centroid_list;                   // sequence numbers of the centroids, ascending
  std::vector<uint32_t> delta_list;                      // the tail of centroid_list the delta index stands for
  size_t main_n = 0, delta_built = 0;                    // centroids in the main index; centroid count when the delta was last built
  KmerAcct kacct;
  if (dev_kmer)
    {
      VsxKmerIndex * a = nullptr, * b = nullptr;
      int irc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &a);
      cix.reset(a);
      if (irc == VSX_OK) { irc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &b); rix.reset(b); }
      if (irc == VSX_OK) { VsxKmerIndex * d = nullptr; irc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &d); dix.reset(d); }
      if (irc != VSX_OK) return irc;
    }

  // unique words of a round's members do not depend on any result: a helper computes them one round ahead (device k-mer path)
  std::vector<std::vector<uint32_t>> pre_kmers;
  uint64_t pre_s0 = UINT64_MAX, pre_main_s0 = UINT64_MAX;
  std::vector<std::vector<Cand>> pre_cands;              // the helper's ranking of the next round against the MAIN centroid index
  std::vector<uint64_t> pre_fallback;
  int pre_rc = VSX_OK;
  std::string pre_err;
  std::vector<uint32_t> main_list;                       // the centroids the main index stands for (a snapshot; see the helper below)
  std::thread pre_thread;
  std::vector<std::vector<uint64_t>> pre_seen;
  auto words_of_round = [&](uint64_t a0, std::vector<std::vector<uint32_t>> & dst, std::vector<std::vector<uint64_t>> & seen, int threads) {
    const uint64_t cnt = std::min<uint64_t>(round, n - a0);
    dst.assign(cnt, {});
    if (seen.size() < (size_t) threads) seen.resize((size_t) threads, std::vector<uint64_t>(S->w < 10 ? (nk + 63) / 64 : 1, 0));
    std::atomic<uint64_t> next {0};
    auto work = [&](int tid) {
      for (;;)
        {
          const uint64_t k = next.fetch_add(16);
          if (k >= cnt) break;
          for (uint64_t x = k; x < std::min(cnt, k + 16); ++x) unique_kmers(seq_of(a0 + x), S->len[a0 + x], S->w, S->o.soft_mask != 0, dst[x], seen[(size_t) tid]);
        }
    };
    run_pool(threads, work);
  };
  struct Joiner { std::thread & t; ~Joiner() { if (t.joinable()) t.join(); } } joiner {pre_thread};
  std::vector<std::vector<uint64_t>> main_seen;
  std::thread reaper;                                    // releases the previous round's host state (see the end of the round loop)
  Joiner reaper_joiner {reaper};

  for (uint64_t s0 = 0; s0 < n; s0 += round)
    {
      const uint64_t wn = std::min<uint64_t>(round, n - s0);
      std::vector<QState> st(wn);
      std::vector<std::vector<uint32_t>> kmers(wn);
      std::vector<uint64_t> fallback;                        // round members the device counters cannot serve

      // ---- phase 1a: k-mer candidates against the centroid index as of the round start ----
      double t0 = now_s();
      if (dev_kmer)
        {
          if (pre_thread.joinable()) pre_thread.join();
          if (pre_rc != VSX_OK) { vsx_internal_set_error(pre_err.c_str()); return pre_rc; }
          const bool have_main = (pre_main_s0 == s0);              // the helper already ranked this round against the main index
          // Take the helper's ranking of THIS round now, before the helper of the next round is started below: that one begins with
          // pre_cands.assign(...), and with tiny rounds (3 sequences: its word stage takes microseconds) it could win the race against
          // the swap that used to sit after its launch -- the round then lost every main-index candidate and its members founded
          // clusters of their own.  Found by oracle/soak_cluster.py in r04 (one round in ~300, GPU round size 3; the r03 library too).
          std::vector<std::vector<Cand>> cands_pre;
          std::vector<uint64_t> fallback_pre;
          if (have_main) { cands_pre.swap(pre_cands); fallback_pre.swap(pre_fallback); }
          if (pre_s0 == s0) kmers.swap(pre_kmers);
          else words_of_round(s0, kmers, main_seen, nth);
          tm_words += now_s() - t0;
          const double tb0 = now_s();
          if (centroid_list.size() != delta_built)
            {
              const size_t total = centroid_list.size();
              if (total - main_n > main_n / 8 + 2 * round)
                {
                  if (have_main) return fail(VSX_EHIP, "vsx_cluster_fast: the main index changed under a prefetched ranking");   // (excluded by the launch condition below)
                  const int irc = vsx_kmer_index_rebuild(cix.get(), centroid_list.data(), total);       // main: everything
                  if (irc != VSX_OK) return irc;
                  main_n = total;
                  main_list.assign(centroid_list.begin(), centroid_list.end());
                  delta_list.clear();
                  static const uint32_t none = 0;                                                        // (a null list would mean "the whole set")
                  const int drc = vsx_kmer_index_rebuild(dix.get(), &none, 0);
                  if (drc != VSX_OK) return drc;
                }
              else
                {
                  delta_list.assign(centroid_list.begin() + (long) main_n, centroid_list.end());
                  const int drc = vsx_kmer_index_rebuild(dix.get(), delta_list.data(), delta_list.size());
                  if (drc != VSX_OK) return drc;
                }
              delta_built = total;
            }
          tm_rebuild += now_s() - tb0;
          // The helper of the NEXT round: its unique words, and -- when this round cannot trigger a rebuild of the main index even if
          // every member founds a cluster -- its ranking against the main index (r03: that ranking is a third of the run and
          // depends on nothing this round decides; only the small delta index has to wait for this round's centroids).  It reads
          // main_list, a snapshot that changes only at a main rebuild, never the growing centroid_list.
          if (s0 + round < n)
            {
              const uint64_t a0 = s0 + round;
              const bool main_safe = main_n > 0 && (centroid_list.size() + wn - main_n) <= main_n / 8 + 2 * round;
              pre_s0 = a0;
              pre_main_s0 = main_safe ? a0 : UINT64_MAX;
              pre_thread = std::thread([&, a0, main_safe]() {
                words_of_round(a0, pre_kmers, pre_seen, std::max(1, nth / 2));
                if (!main_safe) return;
                const uint64_t cnt = std::min<uint64_t>(round, n - a0);
                pre_cands.assign(cnt, {});
                pre_fallback.clear();
                pre_rc = device_rank(S, cix.get(), &main_list, cnt, pre_kmers, (uint32_t) std::max<int64_t>(S->tophits, 1), 1024, true, pre_cands, pre_fallback, kacct,
                                     std::max(1, nth / 2));      // (runs beside the staged search and the near helper)
                if (pre_rc != VSX_OK) pre_err = vsx_last_error();
              });
            }
          const double tr0 = now_s();
          std::vector<std::vector<Cand>> cands(wn);
          const uint32_t keep_n = (uint32_t) std::max<int64_t>(S->tophits, 1);
          int krc = VSX_OK;
          if (have_main) { cands.swap(cands_pre); fallback.swap(fallback_pre); }
          else krc = device_rank(S, cix.get(), &main_list, wn, kmers, keep_n, 1024, true, cands, fallback, kacct);
          if (krc != VSX_OK) return krc;
          if (!delta_list.empty())
            {
              std::vector<std::vector<Cand>> dc(wn);
              std::vector<uint64_t> fb2;
              krc = device_rank(S, dix.get(), &delta_list, wn, kmers, keep_n, 1024, true, dc, fb2, kacct);
              if (krc != VSX_OK) return krc;
              // union of the two selections, the heap's total order, the heap's size
              std::atomic<uint64_t> nx {0};
              auto merge = [&]() {
                for (;;)
                  {
                    const uint64_t k = nx.fetch_add(64);
                    if (k >= wn) break;
                    for (uint64_t x = k; x < std::min<uint64_t>(wn, k + 64); ++x)
                      {
                        if (dc[x].empty()) continue;
                        std::vector<Cand> & c = cands[x];
                        c.insert(c.end(), dc[x].begin(), dc[x].end());
                        const size_t kp = std::min<size_t>(c.size(), (size_t) keep_n);
                        std::partial_sort(c.begin(), c.begin() + (long) kp, c.end(), cand_better);
                        c.resize(kp);
                      }
                  }
              };
              run_pool(std::min(nth, 8), [&](int) { merge(); });
            }
          tm_rank += now_s() - tr0;
          for (uint64_t k = 0; k < wn; ++k) st[k].cands = std::move(cands[k]);
          if (!fallback.empty())
            {
              // the host's growing index is only read here, by the rare queries the device counters cannot serve: it catches up with
              // the centroids founded since its last use (r03: filling it eagerly -- 290 push_backs per centroid -- was a third of the
              // sequential reconcile phase of a 2 M-sequence run)
              std::vector<uint32_t> km;
              std::vector<uint64_t> seen(S->w < 10 ? (nk + 63) / 64 : 1, 0);
              for (; inc.indexed < centroid_list.size(); ++inc.indexed)
                {
                  const uint32_t c = centroid_list[inc.indexed];
                  unique_kmers(seq_of(c), S->len[c], S->w, S->o.soft_mask != 0, km, seen);
                  for (uint32_t w2 : km) inc.post[w2].push_back(c);
                }
            }
          for (uint64_t k : fallback)
            {
              Scratch & sc = scratch[0];
              candidates_for(*S, seq_of(s0 + k), S->len[s0 + k], sc.counts, sc.touched, sc.km, sc.seen, st[k].cands, &inc);
            }
        }
      else
      {
        std::atomic<uint64_t> next {0};
        auto work = [&](int tid) {
          Scratch & sc = scratch[(size_t) tid];
          for (;;)
            {
              const uint64_t k = next.fetch_add(1);
              if (k >= wn) break;
              candidates_for(*S, seq_of(s0 + k), S->len[s0 + k], sc.counts, sc.touched, sc.km, sc.seen, st[k].cands, &inc);
              kmers[k] = sc.km;
            }
        };
        run_pool(nth, work);
      }
      t_kmer += now_s() - t0;

      // ---- phase 1c's device part, started here (r04): the intra-round shared k-mer counts need the round's words only -- nothing
      //      the staged search decides -- so a helper rebuilds the round's own index, counts and pairs up the candidates while phase
      //      1b aligns (k-mer kernels and aligner kernels on their own streams; 1.07 s of a 6.6 s run at 2 M sequences sat behind it) ----
      struct Near { uint32_t k, shared; int64_t res; };            // res = index into the speculative results, -1 none
      std::vector<std::vector<Near>> near(wn);
      std::vector<uint32_t> sq, stg;
      int near_rc = VSX_OK;
      std::string near_err;
      // (the speculative alignments of the fix-up follow the staged search on the same context: aligned by the helper on a second
      //  context beside the search they measured level in r05)
      vsx_results spec;
      std::memset(&spec, 0, sizeof spec);
      struct SpecGuard { vsx_results & r; ~SpecGuard() { vsx_results_free(&r); } } spec_guard {spec};
      const bool near_on_device = dev_kmer && fallback.empty();
      auto near_device = [&]() {
        // the same counting problem on the device: members of the round against an index of the round
        std::vector<uint32_t> round_list(wn);
        for (uint64_t i = 0; i < wn; ++i) round_list[i] = (uint32_t) (s0 + i);
        near_rc = vsx_kmer_index_rebuild(rix.get(), round_list.data(), wn);
        std::vector<std::vector<Cand>> nc(wn);
        std::vector<uint64_t> none;
        if (near_rc == VSX_OK) near_rc = device_rank(S, rix.get(), &round_list, wn, kmers, 0xffffffffu, 1024, false, nc, none, kacct,
                                                     std::max(1, S->threads / 2));      // (beside the staged search: half the budget)
        if (near_rc != VSX_OK) { near_err = vsx_last_error(); return; }
        for (uint64_t i = 0; i < wn; ++i)
          for (const Cand & c : nc[i])                              // ascending target
            {
              const uint32_t k = (uint32_t) (c.target - s0);
              if (k >= i) break;                                    // only earlier members can have become centroids
              Near nr {k, c.count, -1};
              if (acceptable_unaligned(*S, seq_of(s0 + i), S->len[s0 + i], (uint32_t) (s0 + k), S->meta_of(s0 + i)))
                {
                  nr.res = (int64_t) sq.size();
                  sq.push_back((uint32_t) (s0 + i));
                  stg.push_back((uint32_t) (s0 + k));
                }
              near[i].push_back(nr);
            }
      };
      std::thread near_thread;
      struct NearJoiner { std::thread & t; ~NearJoiner() { if (t.joinable()) t.join(); } } near_joiner {near_thread};
      if (near_on_device) near_thread = std::thread(near_device);

      // ---- phase 1b: staged GPU search (queries and targets both live in the database sequence set) ----
      // (no lazy first batches as in vsx_search_batch: a round's plans are latency-bound, and a member whose best centroid fails
      //  pays one more stage -- measured slower in r05)
      const double ts0 = now_s();
      int rc = run_stages(*S, st, [&](uint64_t k) { return seq_of(s0 + k); }, [&](uint64_t k) { return seq_of(s0 + k); },
                          [&](uint64_t k) { return (int64_t) S->len[s0 + k]; },
                          [&](uint64_t k) { return (uint32_t) (s0 + k); }, [&](uint64_t k) { return S->meta_of(s0 + k); }, S->dbset, acct, nullptr, false);
      if (rc != VSX_OK) return rc;
      tm_stages += now_s() - ts0;

      // ---- phase 1c: intra-round shared k-mer counts (unique_count_shared, core/unique.cpp:356-395) and the
      //      speculative alignments of (member i, earlier member k) pairs that the fix-up could ask for ----
      t0 = now_s();
      if (near_on_device)
        {
          near_thread.join();
          if (near_rc != VSX_OK) { vsx_internal_set_error(near_err.c_str()); return near_rc; }
        }
      else
      {
        std::vector<std::vector<uint32_t>> lpost(nk);               // round-local: k-mer -> earlier members
        std::vector<uint16_t> cnt(wn, 0);
        std::vector<uint32_t> touched;
        for (uint64_t i = 0; i < wn; ++i)
          {
            touched.clear();
            for (uint32_t km : kmers[i])
              for (uint32_t k : lpost[km]) { if (cnt[k]++ == 0) touched.push_back(k); }
            std::sort(touched.begin(), touched.end());
            for (uint32_t k : touched)
              {
                Near nr {k, cnt[k], -1};
                cnt[k] = 0;
                if (enough_kmers(*S, nr.shared, (uint32_t) kmers[i].size()) &&
                    acceptable_unaligned(*S, seq_of(s0 + i), S->len[s0 + i], (uint32_t) (s0 + k), S->meta_of(s0 + i)))
                  {
                    nr.res = (int64_t) sq.size();
                    sq.push_back((uint32_t) (s0 + i));
                    stg.push_back((uint32_t) (s0 + k));
                  }
                near[i].push_back(nr);
              }
            for (uint32_t km : kmers[i]) lpost[km].push_back((uint32_t) i);
          }
      }
      t_kmer += now_s() - t0;
      tm_near += now_s() - t0;
      if (!sq.empty())
        {
          t0 = now_s();
          rc = vsx_align_pairs(S->ctx, S->dbset, S->dbset, sq.size(), sq.data(), stg.data(), &spec);
          acct.t_align += now_s() - t0;
          tm_spec += now_s() - t0;
          if (rc != VSX_OK) return rc;
          acct.pairs += sq.size();
        }

      // ---- phase 2: sequential reconciliation in processing order ----
      const double t20 = now_s();
      std::vector<uint32_t> extras;                                  // round members that became centroids, in order
      std::vector<uint8_t> is_extra(wn, 0);
      for (uint64_t i = 0; i < wn; ++i)
        {
          const uint64_t seqno = s0 + i;
          QState & q = st[i];
          const int64_t ql = S->len[seqno];
          std::vector<Hit> & hits = q.hits;

          // evaluate_extra_hits (:601-856)
          int added = 0;
          {
            // candidates = this round's new centroids (extras, increasing) with enough shared words.  A member with words and a
            // positive threshold can only qualify through a near[] entry (shared >= 1), so walk near[i] (sorted by k) and keep the
            // entries that are extras -- the same subsequence the loop over all extras would visit, without its O(extras) cost;
            // members without words (every extra qualifies: enough_kmers with kmersamplecount 0) take the full loop
            auto try_insert = [&](uint32_t k, uint32_t shared) {
              if (!enough_kmers(*S, shared, (uint32_t) kmers[i].size())) return;
              const uint32_t length = S->len[s0 + k];
              int64_t x = (int64_t) hits.size();
              while (x > 0 && ((hits[(size_t) x - 1].count < shared) ||
                               (hits[(size_t) x - 1].count == shared && S->len[hits[(size_t) x - 1].target] > length)))
                --x;
              if (x < hit_capacity)
                {
                  if ((int64_t) hits.size() >= hit_capacity) hits.pop_back();
                  Hit h;
                  h.target = (uint32_t) (s0 + k);
                  h.count = shared;
                  hits.insert(hits.begin() + x, std::move(h));
                  ++added;
                }
            };
            if (!kmers[i].empty() && S->minwordmatches > 0)
              {
                for (const Near & nr : near[i]) if (is_extra[nr.k]) try_insert(nr.k, nr.shared);
              }
            else
              {
                size_t np = 0;                                           // near[i] is sorted by k, extras is increasing too
                for (uint32_t k : extras)
                  {
                    while (np < near[i].size() && near[i][np].k < k) ++np;
                    try_insert(k, (np < near[i].size() && near[i][np].k == k) ? near[i][np].shared : 0);
                  }
              }
          }
          if (added != 0)
            {
              q.rejects = 0; q.accepts = 0;
              for (Hit & h : hits) { h.accepted = false; h.rejected = false; }
              for (size_t t = 0; (q.accepts < S->ma) && (q.rejects < S->mr) && (t < hits.size()); ++t)
                {
                  Hit & h = hits[t];
                  if (!h.aligned)
                    {
                      if (acceptable_unaligned(*S, seq_of(seqno), ql, h.target, S->meta_of(seqno)))
                        {
                          // single-target alignment (:743): taken from the speculative batch when it is there
                          int64_t ri = -1;
                          if (h.target >= s0 && h.target < s0 + wn)
                            for (const Near & nr : near[i]) if (nr.k == h.target - s0) { ri = nr.res; break; }
                          vsx_results one;
                          std::memset(&one, 0, sizeof one);
                          const vsx_results * rp = &spec;
                          if (ri < 0)
                            {
                              const uint32_t a = (uint32_t) seqno, b = h.target;
                              rc = vsx_align_pairs(S->ctx, S->dbset, S->dbset, 1, &a, &b, &one);
                              if (rc != VSX_OK) { vsx_results_free(&spec); return rc; }
                              ++acct.pairs;
                              rp = &one; ri = 0;
                            }
                          acct.cells += (uint64_t) ql * S->len[h.target];
                          rc = fill_hit(*S, [&]() { return seq_of(seqno); }, ql, h, *rp, (uint64_t) ri, acct.sentinels);
                          vsx_results_free(&one);
                          if (rc != VSX_OK) { vsx_results_free(&spec); return fail(rc, "vsx_cluster_fast: fallback aligner failed"); }
                        }
                      else { h.rejected = true; ++q.rejects; }
                    }
                  if (!h.rejected)
                    {
                      if (acceptable_aligned(*S, ql, h, S->abundance(seqno))) ++q.accepts; else ++q.rejects;
                    }
                }
              // delete all undetermined hits from the first one on (:841-854)
              size_t cut = hits.size();
              for (size_t t = hits.size(); t-- > 0;)
                if (!hits[t].accepted && !hits[t].rejected) cut = t;
              hits.resize(cut);
            }

          // search_findbest2_byid / _bysize (searchcore.cpp:960-1025, chosen by --sizeorder, cluster.cpp:1072-1079): first minimum
          // under the comparison, must be accepted
          const Hit * best = nullptr;
          if (S->o.sizeorder) { for (const Hit & h : hits) if (!best || hit_compare_bysize(*S, h, *best) < 0) best = &h; }
          else for (const Hit & h : hits) if (!best || hit_compare_byid(h, *best) < 0) best = &h;
          if (best && !best->accepted) best = nullptr;
          if (best)
            {
              clusterno[seqno] = clusterno[best->target];
              kept_rec.emplace_back();
              hit_record(*best, (uint32_t) seqno, kept_cigar.size(), kept_rec.back());
              kept_cigar.append(best->cigar.c_str(), best->cigar.size() + 1);
            }
          else
            {
              clusterno[seqno] = nclusters++;
              extras.push_back((uint32_t) i);
              is_extra[i] = 1;
              S->is_centroid[seqno] = 1;
              centroid_list.push_back((uint32_t) seqno);
              if (!dev_kmer)
                {
                  for (uint32_t km : kmers[i]) inc.post[km].push_back((uint32_t) seqno);    // Dbindex::add_sequence (:1009); device path: on demand
                  ++inc.indexed;
                }
            }
        }
      vsx_results_free(&spec);
      tm_recon += now_s() - t20;
      // (the round's host state -- 16 384 candidate lists, hit lists, word lists, near lists -- released here so that it shows in the accounting)
      // r06: the round's host state -- 16 384 candidate lists, hit lists, word lists, near lists: ~80 000 heap blocks -- is released on a
      // helper thread beside the next round; on the main thread it was 7.6 ms per round, 0.93 s of a 5.9 s run at 2 M sequences, and in
      // nobody's accounting (profiles/r06/r06g_cluster_phases.txt).
      const double tf0 = now_s();
      if (near_thread.joinable()) near_thread.join();
      if (reaper.joinable()) reaper.join();
      auto * dead_st = new std::vector<QState>(std::move(st));
      auto * dead_km = new std::vector<std::vector<uint32_t>>(std::move(kmers));
      auto * dead_near = new std::vector<std::vector<Near>>(std::move(near));
      reaper = std::thread([dead_st, dead_km, dead_near]() { delete dead_st; delete dead_km; delete dead_near; });
      tm_free += now_s() - tf0;
    }
  if (reaper.joinable()) reaper.join();
  if (std::getenv("VSX_DEBUG_TIMING"))
    std::fprintf(stderr, "vsx_cluster_fast: words %.2f  centroid-index rebuild %.2f  rank vs centroids %.2f  staged search %.2f (align calls %.2f)  "
                         "intra-round counts %.2f  speculative align %.2f  reconcile %.2f  round state released %.2f  total %.2f s\n",
                 tm_words, tm_rebuild, tm_rank, tm_stages, acct.t_align - tm_spec, tm_near, tm_spec, tm_recon, tm_free, now_s() - t_begin);

  {
    vsx_hits * H = &out->hits;
    H->n_queries = n;
    H->n_hits = kept_rec.size();
    H->cigar_bytes = kept_cigar.size();
    H->first = (uint64_t *) std::malloc((n + 1) * sizeof(uint64_t));
    H->hit = (vsx_hit *) std::malloc(std::max<size_t>(kept_rec.size(), 1) * sizeof(vsx_hit));
    H->cigar_blob = (char *) std::malloc(std::max<size_t>(kept_cigar.size(), 1));
    if (!H->first || !H->hit || !H->cigar_blob) { vsx_hits_free(H); return fail(VSX_ENOMEM, "host allocation failed"); }
    if (!kept_rec.empty()) std::memcpy(H->hit, kept_rec.data(), kept_rec.size() * sizeof(vsx_hit));
    if (!kept_cigar.empty()) std::memcpy(H->cigar_blob, kept_cigar.data(), kept_cigar.size());
    // the records are in sequence order, at most one per sequence
    uint64_t at = 0;
    for (uint64_t q = 0; q < n; ++q)
      {
        H->first[q] = at;
        if (at < kept_rec.size() && kept_rec[at].query == q) ++at;
      }
    H->first[n] = at;
    if (at != kept_rec.size()) { vsx_hits_free(H); return fail(VSX_EHIP, "vsx_cluster_fast: hit records out of order"); }
  }
  out->n = n;
  out->n_clusters = nclusters;
  out->clusterno = (uint32_t *) std::malloc(std::max<uint64_t>(n, 1) * sizeof(uint32_t));
  if (!out->clusterno) { vsx_hits_free(&out->hits); return fail(VSX_ENOMEM, "vsx_cluster_fast: host allocation failed"); }
  std::memcpy(out->clusterno, clusterno.data(), n * sizeof(uint32_t));
  out->hits.pairs_aligned = acct.pairs; out->hits.cells_aligned = acct.cells; out->hits.stages = acct.stages;
  out->hits.sentinel_pairs = acct.sentinels; out->hits.seconds_kmer = t_kmer; out->hits.seconds_align = acct.t_align;
  out->hits.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

void vsx_cluster_out_free(vsx_cluster_out * o)
{
  if (!o) return;
  vsx_hits_free(&o->hits);
  std::free(o->clusterno);
  std::memset(o, 0, sizeof *o);
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

// ---- de novo chimera detection's part search (vsx_chimera.cpp, vsx_uchime_denovo) ----------------------------------------------
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
  D->seen.assign(((1ull << (2 * S->w)) + 63) / 64, 0);
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

bool vsx_internal_searcher_has_abundances(const vsx_searcher * S) { return !S->tsize.empty(); }
