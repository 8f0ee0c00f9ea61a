// vsx_chimera.cpp -- --uchime_ref and de novo chimera dispatch (include/vsx_search.h vsx_uchime_ref, vsx_uchime_denovo,
// vsx_chimeras_denovo) and the host restatements of the selection and scoring.  The de novo loop (denovo_window below) reuses steps
// 4-5; its part search lives in vsx_denovo_search.cpp (vsx_internal_denovo_*).  The long-read detector --chimeras_denovo is that loop
// with its own part count, candidate capacity, selection and evaluation (LongMode, align_and_eval_long, vsx_chimera_long.hip).
//
// chimera_process_query (reference core/chimera.cpp:2003-2170) for a WINDOW of queries at a time:
//   1. partition_query (:1930-1955): 4 parts per query of length >= 4 -- offsets into the caller's blob, nothing is copied
//   2. every part of the window through the window search machinery of --usearch_global (vsx_internal_search_parts), searched the
//      way chimera_process_query calls search_onequery (searchcore.cpp:884-957): the part text as given -- no DUST, no --hardmask,
//      only lower-case symbols left out of the k-mers unless qmask is none -- with candidate heaps of maxaccepts + maxrejects
//   3. per query the ACCEPTED hits part by part, repeated targets dropped, first kept (:2017-2071): <= 16 candidates (4 parts x
//      maxaccepts 4).  A query with < 2 candidates, or shorter than the 32-column window, cannot get two parents: answered at once
//   4. one vsx_plan of (whole query, candidate) pairs for the window -- the search16 call of :2076-2087; pairs the 16-bit aligner
//      refuses (sentinel) are realigned with vsx_lma_align (:2094-2131) and their query goes to the host restatement
//   5. vsx_chimera.hip: find_best_parents + eval_parents, one workgroup per query, straight from the plan's hit records and run
//      words in HBM; only the 104-byte result records come back.  Queries above VSX_CHIMERA_MAX_QLEN and sentinel queries:
//      chimera_eval_host below, which is also what VSX_CHIMERA=host runs for every query (A/B and the tests' checker).
#include "../../include/vsx_search.h"
#include "vsx_internal.h"
#include "vsx_private.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using vsxp::fail;
using vsxp::now_s;
using vsxp::map4;
using vsxp::ambiguous4;
using vsxp::DevBuf;

namespace {

thread_local vsx_chimera_stats g_stats {};

constexpr int kParts = 4;            // chimera_info->parts for uchime (:302-304)
constexpr int kWindow = 32;          // `window` (:110)
constexpr uint32_t kNone = 0xFFFFFFFFu;

void unscored(vsx_chimera_result * r, int status, uint32_t pa, uint32_t pb)
{
  std::memset(r, 0, sizeof *r);
  r->parent_a = pa;
  r->parent_b = pb;
  r->closest = kNone;
  r->status = status;
  r->flag = 'N';
}

// CIGAR text (vsx_lma_align) -> run words in text order, (length << 2) | op, op 0 = M, 1 = I, 2 = D
std::vector<uint32_t> runs_from_text(const char * s)
{
  std::vector<uint32_t> out;
  while (*s)
    {
      uint32_t n = 0;
      bool digits = false;
      while (*s >= '0' && *s <= '9') { n = n * 10 + (uint32_t) (*s - '0'); ++s; digits = true; }
      if (!digits) n = 1;
      const char op = *s++;
      out.push_back((n << 2) | (op == 'M' ? 0u : op == 'I' ? 1u : 2u));
    }
  return out;
}

}  // namespace

// find_best_parents (:627-751) + eval_parents (:1245-1700), restated on the host the way the reference computes them: the match
// matrix, the windowed sums over every position, the three-row alignment with the longest insertion before each query position
// (maxi), ignore / diffs per alignment column and the sequential scan with strict '>'.  runs[c] = candidate c's alignment in TEXT
// order; q / t[c] = 4-bit codes.
void vsx_internal_chimera_eval_host(const uint8_t * q, int L, int nc, const uint32_t * cand, const std::vector<std::vector<uint32_t>> & runs,
                                    const std::vector<const uint8_t *> & t, const VsxChimParams & P, vsx_chimera_result * r)
{
  // find_matches
  std::vector<int> match((size_t) nc * (size_t) L, 0);
  for (int i = 0; i < nc; ++i)
    {
      int qpos = 0, tpos = 0;
      for (uint32_t w : runs[i])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 0)
            for (int j = 0; j < len; ++j, ++qpos, ++tpos) { if ((q[qpos] & t[i][tpos]) != 0) match[(size_t) i * L + qpos] = 1; }
          else if (op == 1) tpos += len;
          else qpos += len;
        }
    }
  // find_best_parents
  std::vector<int> smooth((size_t) nc * (size_t) L, 0), maxsmooth((size_t) L, 0);
  int best_parent_cand[2] = {-1, -1};
  std::vector<bool> selected((size_t) nc, false);
  for (int f = 0; f < 2; ++f)
    {
      if (f > 0)
        for (int qpos = kWindow - 1; qpos < L; ++qpos)
          if (smooth[(size_t) best_parent_cand[f - 1] * L + qpos] == maxsmooth[(size_t) qpos])
            for (int i = qpos + 1 - kWindow; i <= qpos; ++i)
              for (int j = 0; j < nc; ++j) match[(size_t) j * L + i] = 0;
      std::fill(maxsmooth.begin(), maxsmooth.end(), 0);
      for (int i = 0; i < nc; ++i)
        if (!selected[(size_t) i])
          {
            int sum = 0;
            for (int qpos = 0; qpos < L; ++qpos)
              {
                const size_t z = (size_t) i * L + qpos;
                sum += match[z];
                if (qpos >= kWindow) sum -= match[z - kWindow];
                if (qpos >= kWindow - 1) { smooth[z] = sum; maxsmooth[(size_t) qpos] = std::max(sum, maxsmooth[(size_t) qpos]); }
              }
          }
      std::vector<int> wins((size_t) nc, 0);
      for (int qpos = kWindow - 1; qpos < L; ++qpos)
        if (maxsmooth[(size_t) qpos] != 0)
          for (int i = 0; i < nc; ++i)
            if (!selected[(size_t) i] && smooth[(size_t) i * L + qpos] == maxsmooth[(size_t) qpos]) ++wins[(size_t) i];
      int maxwins = 0;
      for (int i = 0; i < nc; ++i)
        if (wins[(size_t) i] > maxwins) { maxwins = wins[(size_t) i]; best_parent_cand[f] = i; }
      if (best_parent_cand[f] < 0) break;
      selected[(size_t) best_parent_cand[f]] = true;
    }
  if (best_parent_cand[0] < 0 || best_parent_cand[1] < 0) { unscored(r, VSX_CHIMERA_NO_PARENTS, kNone, kNone); return; }

  // eval_parents: fill_max_alignment_length, the query row, fill_alignment_parents (codes; 0 = '-')
  std::vector<int> maxi((size_t) L + 1, 0);
  for (int p = 0; p < 2; ++p)
    {
      int pos = 0;
      for (uint32_t w : runs[best_parent_cand[p]])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 1) maxi[(size_t) pos] = std::max(len, maxi[(size_t) pos]);
          else pos += len;
        }
    }
  int alnlen = L;
  for (int m : maxi) alnlen += m;
  std::vector<uint8_t> qaln((size_t) alnlen, 0), paln[2];
  for (int i = 0, a = 0; i < L; ++i) { a += maxi[(size_t) i]; qaln[(size_t) a++] = q[i]; }
  for (int p = 0; p < 2; ++p)
    {
      std::vector<uint8_t> & aln = paln[p];
      aln.assign((size_t) alnlen, 0);
      const uint8_t * ts = t[best_parent_cand[p]];
      bool is_inserted = false;
      int qpos = 0, tpos = 0, alnpos = 0;
      for (uint32_t w : runs[best_parent_cand[p]])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 1)
            {
              for (int j = 0; j < maxi[(size_t) qpos]; ++j) aln[(size_t) alnpos++] = j < len ? ts[tpos++] : 0;
              is_inserted = true;
            }
          else
            for (int j = 0; j < len; ++j)
              {
                if (!is_inserted) alnpos += maxi[(size_t) qpos];
                aln[(size_t) alnpos++] = op == 0 ? ts[tpos++] : 0;
                ++qpos;
                is_inserted = false;
              }
        }
    }
  // ignore + diffs ('A' 1, 'B' 2, 'N' / '?' 3, ' ' 0)
  std::vector<bool> ignore((size_t) alnlen, false);
  std::vector<int> diffs((size_t) alnlen, 0);
  for (int i = 0; i < alnlen; ++i)
    {
      const uint8_t qs = qaln[(size_t) i], p1 = paln[0][(size_t) i], p2 = paln[1][(size_t) i];
      if (qs == 0 || p1 == 0 || p2 == 0)
        {
          ignore[(size_t) i] = true;
          if (i > 0) ignore[(size_t) i - 1] = true;
          if (i < alnlen - 1) ignore[(size_t) i + 1] = true;
        }
      if (ambiguous4(qs) || ambiguous4(p1) || ambiguous4(p2)) ignore[(size_t) i] = true;
      int d = 0;
      if (qs != 0 && p1 != 0 && p2 != 0)
        {
          if (p1 == p2) d = qs == p1 ? 0 : 3;
          else d = qs == p1 ? 1 : (qs == p2 ? 2 : 3);
        }
      diffs[(size_t) i] = d;
    }
  int sumA = 0, sumB = 0, sumN = 0;
  for (int i = 0; i < alnlen; ++i)
    {
      if (ignore[(size_t) i]) continue;
      if (diffs[(size_t) i] == 1) ++sumA;
      else if (diffs[(size_t) i] == 2) ++sumB;
      else if (diffs[(size_t) i] != 0) ++sumN;
    }
  int left_n = 0, left_a = 0, left_y = 0, right_n = sumA, right_a = sumN, right_y = sumB;
  double best_h = -1;
  int best_i = -1;
  bool best_is_reverse = false;
  int best_left_y = 0, best_right_y = 0, best_left_n = 0, best_right_n = 0, best_left_a = 0, best_right_a = 0;
  for (int i = 0; i < alnlen; ++i)
    {
      if (ignore[(size_t) i] || diffs[(size_t) i] == 0) continue;
      const int d = diffs[(size_t) i];
      if (d == 1) { ++left_y; --right_n; }
      else if (d == 2) { ++left_n; --right_y; }
      else { ++left_a; --right_a; }
      if ((left_y > left_n) && (right_y > right_n))
        {
          const double left_h = left_y / ((P.xn * (left_n + P.dn)) + left_a);
          const double right_h = right_y / ((P.xn * (right_n + P.dn)) + right_a);
          const double h = left_h * right_h;
          if (h > best_h)
            {
              best_is_reverse = false; best_h = h; best_i = i;
              best_left_n = left_n; best_left_y = left_y; best_left_a = left_a;
              best_right_n = right_n; best_right_y = right_y; best_right_a = right_a;
            }
        }
      else if ((left_n > left_y) && (right_n > right_y))
        {
          const double left_h = left_n / ((P.xn * (left_y + P.dn)) + left_a);
          const double right_h = right_n / ((P.xn * (right_y + P.dn)) + right_a);
          const double h = left_h * right_h;
          if (h > best_h)
            {
              best_is_reverse = true; best_h = h; best_i = i;
              best_left_n = left_y; best_left_y = left_n; best_left_a = left_a;
              best_right_n = right_y; best_right_y = right_n; best_right_a = right_a;
            }
        }
    }
  const uint32_t seq0 = cand[best_parent_cand[0]], seq1 = cand[best_parent_cand[1]];
  if (!(best_h >= 0.0)) { unscored(r, VSX_CHIMERA_NO_ALIGNMENT, seq0, seq1); return; }
  const int ia = best_is_reverse ? 1 : 0, ib = 1 - ia;
  int match_QA = 0, match_QB = 0, match_AB = 0, match_QM = 0, cols = 0;
  for (int i = 0; i < alnlen; ++i)
    {
      if (ignore[(size_t) i]) continue;
      ++cols;
      const uint8_t qs = qaln[(size_t) i], as = paln[ia][(size_t) i], bs = paln[ib][(size_t) i];
      const uint8_t ms = i <= best_i ? as : bs;
      if (qs == as) ++match_QA;
      if (qs == bs) ++match_QB;
      if (as == bs) ++match_AB;
      if (qs == ms) ++match_QM;
    }
  const double QA = 100.0 * match_QA / cols;
  const double QB = 100.0 * match_QB / cols;
  const double AB = 100.0 * match_AB / cols;
  const double QT = std::max(QA, QB);
  const double QM = 100.0 * match_QM / cols;
  const double divdiff = QM - QT;
  const int sumL = best_left_n + best_left_a + best_left_y;
  const int sumR = best_right_n + best_right_a + best_right_y;
  std::memset(r, 0, sizeof *r);
  r->score = best_h;
  r->status = VSX_CHIMERA_SCORED;
  r->parent_a = ia == 0 ? seq0 : seq1;
  r->parent_b = ia == 0 ? seq1 : seq0;
  r->closest = QA >= QB ? r->parent_a : r->parent_b;
  r->id_query_model = QM; r->id_query_a = QA; r->id_query_b = QB; r->id_a_b = AB; r->id_query_top = QT;
  r->left_yes = best_left_y; r->left_no = best_left_n; r->left_abstain = best_left_a;
  r->right_yes = best_right_y; r->right_no = best_right_n; r->right_abstain = best_right_a;
  r->divergence = divdiff;
  r->flag = 'N';
  if (P.variant >= 2)
    {
      if ((match_QM == cols) && (QT < 100.0)) r->flag = 'Y';     // uchime2 / uchime3 (:1633-1640): a perfect model, no '?'
    }
  else if (best_h >= P.minh)
    {
      r->flag = '?';
      if ((divdiff >= P.mindiv) && (sumL >= P.mindiffs) && (sumR >= P.mindiffs)) r->flag = 'Y';
    }
}

namespace {

// scan_matches (:439-502): the longest substring of m[0 .. len) whose score is >= 0, a match scoring pct and a mismatch pct - 100;
// among the longest the leftmost.  Kept in the reference's form, because the sums are doubles and their order of addition decides
// the comparisons: prefix sums p, their suffix maxima q, and two pointers i <= j + 1 where j advances while some end >= j still
// reaches the prefix before i.  A substring of length 0 qualifies (j = i - 1), so the answer is "none" only for len < 1.
bool longest_nonnegative(const uint8_t * m, int len, double pct, std::vector<double> & p, std::vector<double> & q, int * start, int * best_len)
{
  const double gain = pct, cost = pct - 100.0;
  p[0] = 0.0;
  for (int k = 0; k < len; ++k) p[(size_t) k + 1] = p[(size_t) k] + (m[k] ? gain : cost);
  q[(size_t) len] = p[(size_t) len];
  for (int k = len - 1; k >= 0; --k) q[(size_t) k] = std::max(q[(size_t) k + 1], p[(size_t) k]);
  int at = 0, longest = -1;
  double slack = -1.0;
  for (int i = 1, j = 1; j <= len; )
    {
      const double c = q[(size_t) j] - p[(size_t) i - 1];
      if (c >= 0.0)
        {
          if (j - i + 1 > longest) { at = i; longest = j - i + 1; slack = c; }
          ++j;
        }
      else ++i;
    }
  if (!(slack >= 0.0)) return false;
  *start = at - 1;
  *best_len = longest;
  return true;
}

}  // namespace

// find_best_parents_long (:505-624) + eval_parents_long (:995-1242), restated on the host.  runs[c] = candidate c's alignment in
// TEXT order; q / t[c] = 4-bit codes.  The record's parents are cand[] entries.
static void vsx_internal_chimeras_long_eval_host(const uint8_t * q, int L, int nc, const uint32_t * cand, const std::vector<std::vector<uint32_t>> & runs,
                                          const std::vector<const uint8_t *> & t, const VsxChimLongParams & P, vsx_chimeras_long_result * r)
{
  std::memset(r, 0, sizeof *r);
  r->status = VSX_CHIMERA_NO_PARENTS;
  r->flag = 'N';
  // find_matches: a match is a non-zero AND; gapfront = an insertion stands in front of the position (one after the last position
  // is noted by the reference in a cell no round reads, and is left out here)
  std::vector<uint8_t> match((size_t) nc * (size_t) L, 0), gapfront((size_t) nc * (size_t) L, 0);
  for (int c = 0; c < nc; ++c)
    {
      int qpos = 0, tpos = 0;
      for (uint32_t w : runs[(size_t) c])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 0)
            for (int j = 0; j < len; ++j, ++qpos, ++tpos) { if ((q[qpos] & t[(size_t) c][tpos]) != 0) match[(size_t) c * L + qpos] = 1; }
          else if (op == 1) { if (qpos < L) gapfront[(size_t) c * L + qpos] = 1; tpos += len; }
          else qpos += len;
        }
    }
  // rounds: per candidate the segments of unused positions (a used position, or an insertion in front of a position after the
  // segment's first, closes the segment and is skipped), per segment the scan; a longer segment than the best region so far is
  // scanned, a strictly longer region replaces it
  struct Region { int c, start, len; };
  std::vector<Region> found;
  std::vector<uint8_t> used((size_t) L, 0);
  std::vector<double> sp((size_t) L + 1), sq((size_t) L + 1);
  int covered = 0;
  for (int f = 0; f < P.parents_max && f < VSX_CHIMERAS_LONG_MAX_PARENTS; ++f)
    {
      Region best {-1, 0, 0};
      for (int c = 0; c < nc; ++c)
        {
          const uint8_t * m = &match[(size_t) c * L], * g = &gapfront[(size_t) c * L];
          for (int j = 0; j < L; ++j)
            {
              const int start = j;
              while (j < L && !used[(size_t) j] && (j == start || !g[j])) ++j;
              const int seglen = j - start;
              int s = 0, l = 0;
              if (seglen > best.len && longest_nonnegative(m + start, seglen, P.diff_pct, sp, sq, &s, &l) && l > best.len)
                best = Region {c, start + s, l};
            }
        }
      if (best.len < P.length_min) break;
      found.push_back(best);
      std::fill(used.begin() + best.start, used.begin() + best.start + best.len, (uint8_t) 1);
      covered += best.len;
    }
  std::sort(found.begin(), found.end(), [](const Region & a, const Region & b) { return a.start < b.start; });   // (starts are distinct)
  const int np = (int) found.size();
  r->n_parents = np;
  for (int f = 0; f < np; ++f) { r->parent[f] = cand[found[(size_t) f].c]; r->start[f] = found[(size_t) f].start; r->len[f] = found[(size_t) f].len; }
  if (np < 2 || covered != L) return;

  // eval_parents_long.  maxi[p] = the longest insertion in front of position p over the parents (p = L: after the last position)
  std::vector<int> maxi((size_t) L + 1, 0);
  for (const Region & R : found)
    {
      int pos = 0;
      for (uint32_t w : runs[(size_t) R.c])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 1) maxi[(size_t) pos] = std::max(len, maxi[(size_t) pos]);
          else pos += len;
        }
    }
  int gapcols = 0;
  for (int v : maxi) gapcols += v;
  const int alnlen = L + gapcols;
  // columns in which the query's and the parent's codes are EQUAL ('-' has code 0): query positions by comparing codes (a deleted
  // position has parent code 0), insertion columns where the parent has no symbol or one without a code
  double QT = 0.0;
  for (int f = 0; f < np; ++f)
    {
      const int c = found[(size_t) f].c;
      int qpos = 0, tpos = 0, equal = gapcols;
      for (uint32_t w : runs[(size_t) c])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 0)
            for (int j = 0; j < len; ++j, ++qpos, ++tpos) equal += q[qpos] == t[(size_t) c][tpos] ? 1 : 0;
          else if (op == 1)
            for (int j = 0; j < len; ++j, ++tpos) equal -= t[(size_t) c][tpos] != 0 ? 1 : 0;
          else
            for (int j = 0; j < len; ++j, ++qpos) equal += q[qpos] == 0 ? 1 : 0;
        }
      const double QP = 100.0 * equal / alnlen;
      r->id_query_parent[f] = QP;
      QT = std::max(QT, QP);
    }
  r->status = VSX_CHIMERA_CHIMERIC;
  r->flag = 'Y';
  r->alnlen = alnlen;
  r->id_query_top = QT;
  r->divergence = 100.0 * (100.0 - QT) / QT;
}

namespace {

// device buffers of one call, replaced when a window needs more (a hipFree synchronises the whole device)
struct CallBufs {
  DevBuf<VsxPairOut> hits;
  DevBuf<uint32_t> runs;
  DevBuf<VsxChimItem> items;
  DevBuf<vsx_chimera_result> out;
  DevBuf<VsxChimLongItem> long_items;           // --chimeras_denovo
  DevBuf<uint32_t> pair_target;
  DevBuf<vsx_chimeras_long_result> long_out;
  DevBuf<int32_t> long_scratch;                 // the kernel's suffix sums when diff_pct != 0
};

// one query of steps 4-5: its index in the query set of the plan, its text, its candidate parents and where its record goes
template <class Result>
struct EvalJobT {
  uint32_t q;
  const char * text;
  uint32_t len;
  uint32_t ncand;
  const uint32_t * cand;
  Result * out;
};
using EvalJob = EvalJobT<vsx_chimera_result>;
using LongJob = EvalJobT<vsx_chimeras_long_result>;
struct EvalAcct { double t_align = 0, t_eval = 0; uint64_t pairs = 0, sentinels = 0, kernel = 0, host = 0; };

// 4. whole queries against their candidates: one plan of (qidx[p] in qset, tidx[p] in the database set) pairs; its hit records and
// run words are exported into the call's device buffers, the hit records are copied to the host
struct Aligned {
  vsx_plan * plan = nullptr;
  uint64_t npairs = 0, nruns = 0;
  std::vector<VsxPairOut> hits;
  ~Aligned() { vsx_plan_destroy(plan); }
};
int align_pairs(vsx_searcher * S, CallBufs & B, const vsx_seqset * qset, const std::vector<uint32_t> & qidx, const std::vector<uint32_t> & tidx,
                const char * who, Aligned & G)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  int rc = vsx_plan_create(ctx, &G.plan, qset, dbset, qidx.size(), qidx.data(), tidx.data(), 0);
  if (rc == VSX_OK) rc = vsx_plan_run(G.plan);
  if (rc == VSX_OK) rc = vsx_plan_sync(G.plan, nullptr);
  if (rc != VSX_OK) return rc;
  const uint64_t npairs = qidx.size();
  VSX_HIP_AS(who, hipSetDevice(vsx_internal_device(ctx)));
  DevBuf<VsxPairOut> & d_hits = B.hits;
  VSX_HIP_AS(who, d_hits.ensure(npairs));
  rc = vsx_plan_export_hits(G.plan, d_hits.p, npairs * sizeof(VsxPairOut));
  if (rc != VSX_OK) return rc;
  uint64_t nruns = 0;
  rc = vsx_plan_export_runs(G.plan, nullptr, 0, &nruns);          // (the exports themselves re-run a plan whose run buffer overflowed)
  if (rc != VSX_OK) return rc;
  DevBuf<uint32_t> & d_runs = B.runs;
  VSX_HIP_AS(who, d_runs.ensure(std::max<uint64_t>(nruns, 1)));
  if (nruns) { rc = vsx_plan_export_runs(G.plan, d_runs.p, nruns * 4, &nruns); if (rc != VSX_OK) return rc; }
  G.hits.resize(npairs);
  VSX_HIP_AS(who, hipMemcpy(G.hits.data(), d_hits.p, npairs * sizeof(VsxPairOut), hipMemcpyDeviceToHost));
  G.npairs = npairs;
  G.nruns = nruns;

  // every run list the evaluation reads must lie inside the exported buffer: checked here for both routes, so that a bad export
  // fails the call the same way whichever route a query takes (the kernel's own bound check only keeps it inside the buffer)
  for (uint64_t p = 0; p < npairs; ++p)
    if (G.hits[p].score != VSX_SCORE_SENTINEL && G.hits[p].run_off + G.hits[p].nruns > nruns)
      return fail(VSX_EHIP, "%s: run words out of range", who);
  return VSX_OK;
}

// what a host restatement reads of one query: 4-bit codes of the query and its candidates and the alignments' run words in text
// order (pairs the 16-bit aligner refused are realigned with vsx_lma_align)
struct HostQuery {
  std::vector<uint8_t> qcode;
  std::vector<std::vector<uint8_t>> tcode;
  std::vector<std::vector<uint32_t>> runs;
  std::vector<const uint8_t *> tp;
};
int host_query(vsx_searcher * S, const char * qt, uint32_t L, uint32_t nc, const uint32_t * ck, const VsxPairOut * hits,
               const std::vector<uint32_t> & h_runs, HostQuery & H)
{
  const char * dbtext;
  const uint64_t * dboff;
  const uint32_t * dblen;
  vsx_internal_searcher_text(S, &dbtext, &dboff, &dblen);
  const vsx_scoring * sc = vsx_internal_searcher_scoring(S);
  const uint64_t nruns = h_runs.size();
  H.qcode.resize(L);
  for (uint32_t i = 0; i < L; ++i) H.qcode[i] = map4((unsigned char) qt[i]);
  H.runs.assign(nc, {});
  H.tp.resize(nc);
  H.tcode.assign(nc, {});
  for (uint32_t c = 0; c < nc; ++c)
    {
      const char * tt = dbtext + dboff[ck[c]];
      const uint32_t tl = dblen[ck[c]];
      H.tcode[c].resize(tl);
      for (uint32_t i = 0; i < tl; ++i) H.tcode[c][i] = map4((unsigned char) tt[i]);
      H.tp[c] = H.tcode[c].data();
      const VsxPairOut & h = hits[c];
      if (h.score == VSX_SCORE_SENTINEL)
        {
          int64_t score, alen, ma, mi, ga;
          char * cig = nullptr;
          const int rc = vsx_lma_align(sc, qt, L, tt, tl, &score, &alen, &ma, &mi, &ga, &cig);
          if (rc != VSX_OK) return rc;
          H.runs[c] = runs_from_text(cig);
          std::free(cig);
        }
      else
        {
          H.runs[c].assign(h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off - h.nruns), h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off));
        }
    }
  return VSX_OK;
}

// 4-5 for --uchime_ref and the uchime de novo forms: selection + scoring on the kernel, or on the host restatement (long query,
// sentinel pair, host_all).  A job with < 2 candidates, or shorter than the 32-column window, cannot get two parents and is answered
// at once.
int align_and_eval(vsx_searcher * S, const VsxChimParams & P, CallBufs & B, bool host_all, const vsx_seqset * qset,
                   const std::vector<EvalJob> & jobs, EvalAcct & A, const char * who)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  const double t1 = now_s();
  const size_t nj = jobs.size();
  std::vector<uint32_t> qidx, tidx, pair0(nj, 0);
  std::vector<bool> scored(nj, false);
  for (size_t k = 0; k < nj; ++k)
    {
      const EvalJob & j = jobs[k];
      if (j.ncand < 2 || j.len < (uint32_t) kWindow) { unscored(j.out, VSX_CHIMERA_NO_PARENTS, kNone, kNone); continue; }
      scored[k] = true;
      pair0[k] = (uint32_t) qidx.size();
      for (uint32_t c = 0; c < j.ncand; ++c) { qidx.push_back(j.q); tidx.push_back(j.cand[c]); }
    }
  if (qidx.empty()) return VSX_OK;

  Aligned G;
  int rc = align_pairs(S, B, qset, qidx, tidx, who, G);
  if (rc != VSX_OK) return rc;
  const std::vector<VsxPairOut> & h_hits = G.hits;
  const uint64_t nruns = G.nruns;
  DevBuf<VsxPairOut> & d_hits = B.hits;
  DevBuf<uint32_t> & d_runs = B.runs;
  const double t2 = now_s();
  A.t_align += t2 - t1;
  A.pairs += G.npairs;

  // 5. route: kernel, or host restatement (long query, sentinel pair, VSX_CHIMERA=host)
  std::vector<VsxChimItem> items;
  std::vector<size_t> item_job, host_q;
  for (size_t k = 0; k < nj; ++k)
    {
      if (!scored[k]) continue;
      const EvalJob & j = jobs[k];
      bool sentinel = false;
      for (uint32_t c = 0; c < j.ncand; ++c)
        if (h_hits[pair0[k] + c].score == VSX_SCORE_SENTINEL) { sentinel = true; ++A.sentinels; }
      if (host_all || sentinel || j.len > VSX_CHIMERA_MAX_QLEN) { host_q.push_back(k); continue; }
      VsxChimItem it {};
      it.q = j.q;
      it.ncand = j.ncand;
      it.pair0 = pair0[k];
      it.out = (uint32_t) items.size();
      std::copy(j.cand, j.cand + j.ncand, it.cand);
      items.push_back(it);
      item_job.push_back(k);
    }
  if (!items.empty())
    {
      const uint8_t * qc, * tc;
      const uint64_t * qo, * to;
      const uint32_t * ql, * tl;
      uint64_t dummy;
      vsx_internal_seqset_device(qset, &qc, &qo, &ql, &dummy);
      vsx_internal_seqset_device(dbset, &tc, &to, &tl, &dummy);
      hipStream_t st = vsx_internal_stream(ctx);
      DevBuf<VsxChimItem> & d_items = B.items;
      DevBuf<vsx_chimera_result> & d_out = B.out;
      VSX_HIP_AS(who, d_items.ensure(items.size()));
      VSX_HIP_AS(who, d_out.ensure(items.size()));
      VSX_HIP_AS(who, hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(VsxChimItem), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(who, vsx_launch_chimera_eval(d_items.p, (uint32_t) items.size(), qc, qo, ql, tc, to, tl, d_hits.p, d_runs.p, nruns, P, d_out.p, st));
      std::vector<vsx_chimera_result> res(items.size());
      VSX_HIP_AS(who, hipMemcpyAsync(res.data(), d_out.p, res.size() * sizeof(vsx_chimera_result), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(who, hipStreamSynchronize(st));
      for (size_t x = 0; x < items.size(); ++x) *jobs[item_job[x]].out = res[items[x].out];
      A.kernel += items.size();
    }
  if (!host_q.empty())
    {
      std::vector<uint32_t> h_runs(nruns);
      if (nruns) VSX_HIP_AS(who, hipMemcpy(h_runs.data(), d_runs.p, nruns * 4, hipMemcpyDeviceToHost));
      HostQuery H;
      for (size_t k : host_q)
        {
          const EvalJob & j = jobs[k];
          rc = host_query(S, j.text, j.len, j.ncand, j.cand, &h_hits[pair0[k]], h_runs, H);
          if (rc != VSX_OK) return rc;
          vsx_internal_chimera_eval_host(H.qcode.data(), (int) j.len, (int) j.ncand, j.cand, H.runs, H.tp, P, j.out);
        }
      A.host += host_q.size();
    }
  A.t_eval += now_s() - t2;
  return VSX_OK;
}

// 4-5 for --chimeras_denovo.  A job without candidates has no parents and is answered at once; the kernel takes what the header
// states (length, candidate count, no sentinel pair, diff_pct a multiple of 2^-13), the host restatement everything else.
int align_and_eval_long(vsx_searcher * S, const VsxChimLongParams & P, CallBufs & B, bool host_all, const vsx_seqset * qset,
                        const std::vector<LongJob> & jobs, EvalAcct & A, const char * who)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  const double t1 = now_s();
  const size_t nj = jobs.size();
  std::vector<uint32_t> qidx, tidx, pair0(nj, 0);
  for (size_t k = 0; k < nj; ++k)
    {
      const LongJob & j = jobs[k];
      pair0[k] = (uint32_t) qidx.size();
      if (j.ncand == 0) { std::memset(j.out, 0, sizeof *j.out); j.out->status = VSX_CHIMERA_NO_PARENTS; j.out->flag = 'N'; }
      for (uint32_t c = 0; c < j.ncand; ++c) { qidx.push_back(j.q); tidx.push_back(j.cand[c]); }
    }
  if (qidx.empty()) return VSX_OK;

  Aligned G;
  int rc = align_pairs(S, B, qset, qidx, tidx, who, G);
  if (rc != VSX_OK) return rc;
  const uint64_t nruns = G.nruns;
  const double t2 = now_s();
  A.t_align += t2 - t1;
  A.pairs += G.npairs;

  // the kernel scans in units of 2^-13: it takes the call iff diff_pct * 2^13 is an integer (include/vsx_search.h)
  VsxChimLongParams K = P;
  const double units = P.diff_pct * 8192.0;
  const bool scaled = units == (double) (int32_t) units;
  K.gain = scaled ? (int32_t) units : 0;
  std::vector<VsxChimLongItem> items;
  std::vector<size_t> item_job, host_q;
  for (size_t k = 0; k < nj; ++k)
    {
      const LongJob & j = jobs[k];
      if (j.ncand == 0) continue;
      bool sentinel = false;
      for (uint32_t c = 0; c < j.ncand; ++c)
        if (G.hits[pair0[k] + c].score == VSX_SCORE_SENTINEL) { sentinel = true; ++A.sentinels; }
      if (host_all || sentinel || !scaled || j.len > VSX_CHIMERAS_LONG_MAX_QLEN || j.ncand > VSX_CHIMERAS_LONG_MAX_CAND)
        { host_q.push_back(k); continue; }
      items.push_back(VsxChimLongItem {j.q, j.ncand, pair0[k], (uint32_t) items.size()});
      item_job.push_back(k);
    }
  if (!items.empty())
    {
      const uint8_t * qc, * tc;
      const uint64_t * qo, * to;
      const uint32_t * ql, * tl;
      uint64_t dummy;
      vsx_internal_seqset_device(qset, &qc, &qo, &ql, &dummy);
      vsx_internal_seqset_device(dbset, &tc, &to, &tl, &dummy);
      hipStream_t st = vsx_internal_stream(ctx);
      VSX_HIP_AS(who, B.long_items.ensure(items.size()));
      VSX_HIP_AS(who, B.long_out.ensure(items.size()));
      VSX_HIP_AS(who, B.pair_target.ensure(tidx.size()));
      VSX_HIP_AS(who, hipMemcpyAsync(B.long_items.p, items.data(), items.size() * sizeof(VsxChimLongItem), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(who, hipMemcpyAsync(B.pair_target.p, tidx.data(), tidx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      if (K.gain != 0) VSX_HIP_AS(who, B.long_scratch.ensure(VSX_CHIMLONG_SCRATCH_GROUPS * VSX_CHIMLONG_SCRATCH_INTS));
      VSX_HIP_AS(who, vsx_launch_chimeras_long(B.long_items.p, (uint32_t) items.size(), qc, qo, ql, tc, to, tl, B.hits.p, B.pair_target.p,
                                                 G.npairs, B.runs.p, nruns, K, K.gain != 0 ? B.long_scratch.p : nullptr, B.long_out.p, st));
      std::vector<vsx_chimeras_long_result> res(items.size());
      VSX_HIP_AS(who, hipMemcpyAsync(res.data(), B.long_out.p, res.size() * sizeof(vsx_chimeras_long_result), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(who, hipStreamSynchronize(st));
      for (size_t x = 0; x < items.size(); ++x) *jobs[item_job[x]].out = res[items[x].out];
      A.kernel += items.size();
    }
  if (!host_q.empty())
    {
      std::vector<uint32_t> h_runs(nruns);
      if (nruns) VSX_HIP_AS(who, hipMemcpy(h_runs.data(), B.runs.p, nruns * 4, hipMemcpyDeviceToHost));
      HostQuery H;
      for (size_t k : host_q)
        {
          const LongJob & j = jobs[k];
          rc = host_query(S, j.text, j.len, j.ncand, j.cand, &G.hits[pair0[k]], h_runs, H);
          if (rc != VSX_OK) return rc;
          vsx_internal_chimeras_long_eval_host(H.qcode.data(), (int) j.len, (int) j.ncand, j.cand, H.runs, H.tp, P, j.out);
        }
      A.host += host_q.size();
    }
  A.t_eval += now_s() - t2;
  return VSX_OK;
}

// the `parts` parts of a query of length L >= parts (partition_query, :1930-1955): lengths of the integer split, front to back
template <class F>
void for_each_part(uint32_t L, int parts, F && f)
{
  uint32_t rest = L, at = 0;
  for (int i = 0; i < parts; ++i)
    {
      const uint32_t length = (rest + (uint32_t) (parts - i - 1)) / (uint32_t) (parts - i);
      f(at, length);
      rest -= length;
      at += length;
    }
}

// one window: queries [w0, w0 + nw) of the call
int run_window(vsx_searcher * S, const vsx_chimera_opts & O, CallBufs & B, bool host_all, uint64_t w0, uint64_t nw, const char * qblob, uint64_t qbytes,
               const uint64_t * qoff, const uint32_t * qlen, vsx_chimera_result * out)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const VsxChimParams P {O.minh, O.mindiv, O.xn, O.dn, O.mindiffs, 0};
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);

  // 1-2. parts through the window search
  double t0 = now_s();
  std::vector<uint64_t> poff;
  std::vector<uint32_t> plen, pquery;
  for (uint64_t k = 0; k < nw; ++k)
    {
      const uint32_t L = qlen[w0 + k];
      if (L < (uint32_t) kParts) continue;
      for_each_part(L, kParts, [&](uint32_t at, uint32_t length) { poff.push_back(qoff[w0 + k] + at); plen.push_back(length); pquery.push_back((uint32_t) k); });
    }
  std::vector<uint32_t> ncand(nw, 0), cand(nw * VSX_CHIM_MAXCAND, 0);
  if (!poff.empty())
    {
      vsx_hits H {};
      const int rc = vsx_internal_search_parts(S, so.maxaccepts + so.maxrejects, poff.size(), qblob, qbytes, poff.data(), plen.data(), &H);
      if (rc != VSX_OK) return rc;
      // 3. accepted hits part by part, best first; repeated targets dropped
      for (uint64_t p = 0; p < poff.size(); ++p)
        {
          const uint32_t k = pquery[p];
          uint32_t * c = &cand[(size_t) k * VSX_CHIM_MAXCAND];
          for (uint64_t h = H.first[p]; h < H.first[p + 1]; ++h)
            {
              if (!H.hit[h].accepted) continue;
              const uint32_t tg = H.hit[h].target;
              if (std::find(c, c + ncand[k], tg) == c + ncand[k] && ncand[k] < VSX_CHIM_MAXCAND) c[ncand[k]++] = tg;
            }
        }
      g_stats.parts += poff.size();
      vsx_hits_free(&H);
    }
  g_stats.seconds_search += now_s() - t0;

  // 4-5. whole queries against their candidates (one plan for the window), selection + scoring
  std::vector<uint64_t> woff(nw);
  std::string wblob;
  std::vector<EvalJob> jobs(nw);
  for (uint64_t k = 0; k < nw; ++k)
    {
      woff[k] = wblob.size();
      wblob.append(qblob + qoff[w0 + k], qlen[w0 + k]);
      jobs[k] = EvalJob {(uint32_t) k, qblob + qoff[w0 + k], qlen[w0 + k], ncand[k], &cand[(size_t) k * VSX_CHIM_MAXCAND], &out[w0 + k]};
    }
  bool any = false;
  for (uint64_t k = 0; k < nw && !any; ++k) any = ncand[k] >= 2 && qlen[w0 + k] >= (uint32_t) kWindow;
  if (!any)
    {
      for (const EvalJob & j : jobs) unscored(j.out, VSX_CHIMERA_NO_PARENTS, kNone, kNone);
      return VSX_OK;
    }
  vsx_seqset * qs = nullptr;
  int rc = vsx_seqset_create(ctx, &qs, nw, wblob.data(), wblob.size(), woff.data(), qlen + w0);
  if (rc != VSX_OK) return rc;
  struct Guard { vsx_seqset * s; ~Guard() { vsx_seqset_destroy(s); } } g {qs};
  EvalAcct A;
  rc = align_and_eval(S, P, B, host_all, qs, jobs, A, "vsx_uchime_ref");
  g_stats.seconds_align += A.t_align;
  g_stats.pairs_aligned += A.pairs;
  g_stats.sentinel_pairs += A.sentinels;
  g_stats.queries_kernel += A.kernel;
  g_stats.queries_host += A.host;
  g_stats.seconds_eval += A.t_eval;
  return rc;
}

}  // namespace

namespace {

thread_local vsx_chimera_denovo_stats g_dstats {}, g_lstats {};

// the uchime forms: 4 parts of a query of length >= 4, <= 16 candidates
struct UchimeMode {
  using Result = vsx_chimera_result;
  VsxChimParams P;
  CallBufs & B;
  bool host_all;
  int parts(uint32_t L) const { return L >= (uint32_t) kParts ? kParts : 0; }
  uint32_t capacity(int) const { return VSX_CHIM_MAXCAND; }
  // status < suspicious (chimera.cpp:2314, :2365): what joins the index of later queries
  bool keeps(const Result & r) const { return r.flag == 'N'; }
  int eval(vsx_searcher * S, const std::vector<EvalJob> & jobs, EvalAcct & A)
  { return align_and_eval(S, P, B, host_all, vsx_internal_searcher_dbset(S), jobs, A, "vsx_uchime_denovo"); }
};

// --chimeras_denovo: (length + 99) / 100 parts, or the given number, within 2 .. 100 (realloc_arrays, :285-299); a query shorter than
// its part count is not searched (:2018); maxaccepts accepted hits per part
struct LongMode {
  using Result = vsx_chimeras_long_result;
  VsxChimLongParams P;
  int32_t parts_opt;
  uint32_t maxaccepts;
  CallBufs & B;
  bool host_all;
  int parts(uint32_t L) const
  {
    const int64_t n = parts_opt ? parts_opt : ((int64_t) L + 99) / 100;
    const int p = (int) std::min<int64_t>(std::max<int64_t>(n, 2), 100);
    return L >= (uint32_t) p ? p : 0;
  }
  uint32_t capacity(int parts) const { return maxaccepts * (uint32_t) parts; }
  // the only statuses are chimeric and no_parents; what is not chimeric joins the index (:2365-2371)
  bool keeps(const Result & r) const { return r.flag != 'Y'; }
  int eval(vsx_searcher * S, const std::vector<LongJob> & jobs, EvalAcct & A)
  { return align_and_eval_long(S, P, B, host_all, vsx_internal_searcher_dbset(S), jobs, A, "vsx_chimeras_denovo"); }
};

// One window [s0, s0 + wn) of vsx_uchime_denovo / vsx_chimeras_denovo: speculative passes with an in-order fix-up.
//   present[j]  member j's assumed status in the current pass: its final one when resolved, "non-chimera" while pending
//   lists[p]    part p's merged candidate list of the pass that produced the query's current result
//   deps[k]     the earlier members that appeared in one of query k's lists
// A pass re-searches, re-aligns and re-evaluates only the pending queries whose lists changed; a pending query whose lists did not
// change keeps its result (the same lists give the same search, the same parents and the same scores).  A member reaches a list only
// while it is assumed present, so query k is final once every member in deps[k] is final and a non-chimera: a member that did not
// reach a list could only have pushed others out, and a pending member assumed present that turns out chimeric leaves the lists it
// was not in unchanged.  The first pending query sees only final members, so every pass resolves at least one query.
// Mode says what differs between the uchime forms and --chimeras_denovo: the parts of a query of a given length (0 = not searched),
// the most candidates a query with that many parts can collect, steps 4-5, and which records join the index.
template <class Mode>
int denovo_window(vsx_searcher * S, VsxDenovo * D, Mode & M, vsx_chimera_denovo_stats & st, uint64_t s0, uint64_t wn,
                  typename Mode::Result * out, std::vector<uint32_t> & commit)
{
  const char * text;
  const uint64_t * off;
  const uint32_t * len;
  vsx_internal_searcher_text(S, &text, &off, &len);

  std::vector<uint64_t> poff;
  std::vector<uint32_t> plen, pmember, part0(wn + 1, 0), cand0(wn + 1, 0);
  for (uint64_t k = 0; k < wn; ++k)
    {
      part0[k] = (uint32_t) poff.size();
      const uint32_t L = len[s0 + k];
      const int parts = M.parts(L);
      cand0[k + 1] = cand0[k] + M.capacity(parts);
      if (parts > 0)
        for_each_part(L, parts, [&](uint32_t at, uint32_t length) { poff.push_back(off[s0 + k] + at); plen.push_back(length); pmember.push_back((uint32_t) k); });
    }
  part0[wn] = (uint32_t) poff.size();
  st.parts += poff.size();
  int rc = vsx_internal_denovo_window(D, s0, wn, poff, plen, pmember, &st.seconds_rank, &st.seconds_members);
  if (rc != VSX_OK) return rc;

  std::vector<uint8_t> present(wn, 1), final_(wn, 0), done_once(wn, 0);
  std::vector<std::vector<uint32_t>> lists(poff.size()), deps(wn);
  std::vector<uint32_t> ncand(wn, 0), cand(cand0[wn], 0);
  std::vector<uint32_t> pending(wn);
  for (uint64_t k = 0; k < wn; ++k) pending[k] = (uint32_t) k;
  uint64_t passes = 0;
  std::vector<uint32_t> tl;
  while (!pending.empty())
    {
      ++passes;
      // which pending queries have new lists
      double t0 = now_s();
      std::vector<uint32_t> redo, parts;
      for (uint32_t k : pending)
        {
          bool changed = !done_once[k];
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p)
            {
              vsx_internal_denovo_merge(D, p, present.data(), tl);
              if (tl != lists[p]) { changed = true; lists[p].swap(tl); }
            }
          if (!changed) continue;
          if (done_once[k]) ++st.queries_reevaluated;
          done_once[k] = 1;
          redo.push_back(k);
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p) parts.push_back(p);
          deps[k].clear();
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p)
            for (uint32_t t : lists[p])
              if (t >= s0 && std::find(deps[k].begin(), deps[k].end(), (uint32_t) (t - s0)) == deps[k].end()) deps[k].push_back((uint32_t) (t - s0));
        }
      st.seconds_reconcile += now_s() - t0;

      // the parts of those queries through the staged search; accepted hits part by part, repeated targets dropped (:2017-2071)
      t0 = now_s();
      std::vector<std::vector<uint32_t>> acc;
      rc = vsx_internal_denovo_search(D, parts, acc, &st.pairs_searched, &st.sentinel_pairs);
      if (rc != VSX_OK) return rc;
      st.seconds_search += now_s() - t0;
      size_t x = 0;
      for (uint32_t k : redo)
        {
          ncand[k] = 0;
          uint32_t * c = cand.data() + cand0[k];
          const uint32_t cap = cand0[k + 1] - cand0[k];
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p, ++x)
            for (uint32_t tg : acc[x])
              if (std::find(c, c + ncand[k], tg) == c + ncand[k] && ncand[k] < cap) c[ncand[k]++] = tg;
        }

      // whole queries (in the database set) against their candidates, selection + scoring
      if (!redo.empty())
        {
          std::vector<EvalJobT<typename Mode::Result>> jobs;
          jobs.reserve(redo.size());
          for (uint32_t k : redo)
            jobs.push_back(EvalJobT<typename Mode::Result> {(uint32_t) (s0 + k), text + off[s0 + k], len[s0 + k], ncand[k], cand.data() + cand0[k], &out[s0 + k]});
          EvalAcct A;
          rc = M.eval(S, jobs, A);
          if (rc != VSX_OK) return rc;
          st.seconds_align += A.t_align;
          st.seconds_eval += A.t_eval;
          st.pairs_aligned += A.pairs;
          st.sentinel_pairs += A.sentinels;
          st.queries_kernel += A.kernel;
          st.queries_host += A.host;
        }

      // validate in order
      t0 = now_s();
      std::vector<uint32_t> still;
      for (uint32_t k : pending)
        {
          bool ok = true;
          for (uint32_t j : deps[k])
            if (!final_[j] || !M.keeps(out[s0 + j])) { ok = false; break; }          // (a member in a list was assumed present)
          if (ok) { final_[k] = 1; present[k] = M.keeps(out[s0 + k]) ? 1 : 0; }
          else still.push_back(k);
        }
      pending.swap(still);
      st.seconds_reconcile += now_s() - t0;
    }
  st.passes += passes;
  st.passes_max = std::max<uint64_t>(st.passes_max, passes);
  for (uint64_t k = 0; k < wn; ++k)
    if (present[k]) commit.push_back((uint32_t) (s0 + k));
  return VSX_OK;
}

}  // namespace

// align_pairs for vsx_chimalns.cpp (vsx_private.h): the same call, with buffers the handle owns
struct VsxRealigned {
  CallBufs bufs;
  Aligned aligned;
};

int vsx_internal_chimera_realign(vsx_searcher * S, const vsx_seqset * qset, const std::vector<uint32_t> & qidx, const std::vector<uint32_t> & tidx,
                                 const char * who, VsxRealigned ** out)
{
  VsxRealigned * R = new VsxRealigned;
  *out = R;
  return align_pairs(S, R->bufs, qset, qidx, tidx, who, R->aligned);
}

void vsx_internal_chimera_realigned_view(const VsxRealigned * R, const VsxPairOut ** hits, const uint32_t ** d_runs, uint64_t * nruns)
{
  *hits = R->aligned.hits.data();
  *d_runs = R->bufs.runs.p;
  *nruns = R->aligned.nruns;
}

void vsx_internal_chimera_realigned_free(VsxRealigned * R) { delete R; }

extern "C" {

void vsx_chimera_opts_default(vsx_chimera_opts * o)
{
  std::memset(o, 0, sizeof *o);
  vsx_search_opts_default(&o->search);
  o->search.id = 0.55;                  // chimera_id
  o->search.weak_id = 0.55;
  o->search.maxaccepts = 4;             // few
  o->search.maxrejects = 16;            // rejects
  o->search.soft_mask = 2;              // --dbmask dust, the reference's default
  o->minh = 0.28;
  o->mindiv = 0.8;
  o->mindiffs = 3;
  o->xn = 8.0;
  o->dn = 1.4;
}

void vsx_chimera_last_stats(vsx_chimera_stats * out) { if (out) *out = g_stats; }

int vsx_uchime_ref(vsx_searcher * S, const vsx_chimera_opts * O, uint64_t n, const char * qblob, uint64_t qbytes,
                   const uint64_t * qoff, const uint32_t * qlen, vsx_chimera_result * out)
{
  g_stats = vsx_chimera_stats {};
  const double t0 = now_s();
  if (!S || !O || (n && (!qblob || !qoff || !qlen || !out))) return fail(VSX_EINVAL, "vsx_uchime_ref: null argument");
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);
  if (so.id != 0.55 || so.weak_id != 0.55 || so.maxaccepts != 4 || so.maxrejects != 16 || so.strand_both || so.cluster_unoise || so.self)
    return fail(VSX_EINVAL, "vsx_uchime_ref: the searcher was not created with the detection parameters (vsx_chimera_opts_default: "
                             "id = weak_id = 0.55, maxaccepts 4, maxrejects 16, plus strand)");
  if (O->mindiffs < 0 || !(O->xn > 0.0) || !(O->dn >= 0.0)) return fail(VSX_EINVAL, "vsx_uchime_ref: xn must be > 0, dn >= 0, mindiffs >= 0");
  if (const int rc = vsxp::check_spans("vsx_uchime_ref", "query", n, qoff, qlen, qbytes)) return rc;
  const bool host_all = vsxp::env_is_host("VSX_CHIMERA");
  const uint64_t window = O->window > 0 ? (uint64_t) O->window : 16384;
  CallBufs bufs;
  for (uint64_t w0 = 0; w0 < n; w0 += window)
    {
      const int rc = run_window(S, *O, bufs, host_all, w0, std::min(window, n - w0), qblob, qbytes, qoff, qlen, out);
      if (rc != VSX_OK) return rc;
      ++g_stats.windows;
    }
  g_stats.seconds_total = now_s() - t0;
  return VSX_OK;
}

void vsx_chimera_denovo_opts_default(vsx_chimera_denovo_opts * o, int32_t variant)
{
  std::memset(o, 0, sizeof *o);
  vsx_chimera_opts_default(&o->base);
  o->variant = variant;
  o->abskew = variant == 3 ? 16.0 : 2.0;          // cli.cc:4478-4492
  o->base.search.self = 1;                          // chimera_detection_parameters (chimera.cpp:2805-2824)
  o->base.search.selfid = 1;
  o->base.search.maxsizeratio = 1.0 / o->abskew;
}

void vsx_chimera_denovo_last_stats(vsx_chimera_denovo_stats * out) { if (out) *out = g_dstats; }

int vsx_uchime_denovo(vsx_searcher * S, const vsx_chimera_denovo_opts * O, vsx_chimera_result * out)
{
  g_dstats = vsx_chimera_denovo_stats {};
  const double t0 = now_s();
  if (!O) return fail(VSX_EINVAL, "vsx_uchime_denovo: null options");
  if (O->variant < 1 || O->variant > 3) return fail(VSX_EINVAL, "vsx_uchime_denovo: variant must be 1 (uchime), 2 (uchime2) or 3 (uchime3)");
  if (!(O->abskew >= 1.0)) return fail(VSX_EINVAL, "vsx_uchime_denovo: abskew must be >= 1.0");
  if (O->base.mindiffs < 0 || !(O->base.xn > 0.0) || !(O->base.dn >= 0.0))
    return fail(VSX_EINVAL, "vsx_uchime_denovo: xn must be > 0, dn >= 0, mindiffs >= 0");
  if (!S || !out) return fail(VSX_EINVAL, "vsx_uchime_denovo: null argument");
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);
  if (so.strand_both) return fail(VSX_EINVAL, "vsx_uchime_denovo: --strand both is not provided (the reference refuses it)");
  if (so.id != 0.55 || so.weak_id != 0.55 || so.maxaccepts != 4 || so.maxrejects != 16 || so.cluster_unoise || so.self != 1 ||
      so.selfid != 1 || so.maxsizeratio != 1.0 / O->abskew || (so.qmask != 0 && so.qmask != so.soft_mask + 1))
    return fail(VSX_EINVAL, "vsx_uchime_denovo: the searcher was not created with the detection parameters (vsx_chimera_denovo_opts_default: "
                             "id = weak_id = 0.55, maxaccepts 4, maxrejects 16, self = selfid = 1, maxsizeratio = 1 / abskew, qmask as soft_mask)");
  if (!vsx_internal_searcher_has_abundances(S)) return fail(VSX_EINVAL, "vsx_uchime_denovo: the searcher has no abundances (vsx_searcher_set_meta)");
  if (so.wordlength > 8) return fail(VSX_EINVAL, "vsx_uchime_denovo: word lengths above 8 are not provided");
  const char * text;
  const uint64_t * off;
  const uint32_t * len;
  vsx_internal_searcher_text(S, &text, &off, &len);
  const uint64_t n = vsx_seqset_count(vsx_internal_searcher_dbset(S));
  if (n == 0) { g_dstats.seconds_total = now_s() - t0; return VSX_OK; }
  VsxDenovo * D = nullptr;
  int rc = vsx_internal_denovo_create(S, &D);
  if (rc != VSX_OK) return rc;
  struct DGuard { VsxDenovo * d; ~DGuard() { vsx_internal_denovo_destroy(d); } } dg {D};
  const bool host_all = vsxp::env_is_host("VSX_CHIMERA");
  const uint64_t window = O->base.window > 0 ? (uint64_t) O->base.window : 4096;
  CallBufs bufs;
  UchimeMode mode {VsxChimParams {O->base.minh, O->base.mindiv, O->base.xn, O->base.dn, O->base.mindiffs, O->variant}, bufs, host_all};
  std::vector<uint32_t> commit;
  for (uint64_t s0 = 0; s0 < n; s0 += window)
    {
      commit.clear();
      rc = denovo_window(S, D, mode, g_dstats, s0, std::min(window, n - s0), out, commit);
      if (rc != VSX_OK) return rc;
      vsx_internal_denovo_commit(D, commit);
      ++g_dstats.windows;
    }
  g_dstats.seconds_total = now_s() - t0;
  return VSX_OK;
}

void vsx_chimeras_long_opts_default(vsx_chimeras_long_opts * o)
{
  std::memset(o, 0, sizeof *o);
  vsx_chimera_denovo_opts d;
  vsx_chimera_denovo_opts_default(&d, 1);
  o->search = d.base.search;
  o->parts = 0;
  o->parents_max = 3;
  o->length_min = 10;
  o->diff_pct = 0.0;
  o->abskew = 1.0;                                  // cli.cc:4481-4484
  o->search.maxsizeratio = 1.0 / o->abskew;
}

void vsx_chimeras_denovo_last_stats(vsx_chimera_denovo_stats * out) { if (out) *out = g_lstats; }

static int chimeras_long_check(const vsx_chimeras_long_opts * O, const char * who)
{
  if (!O) return fail(VSX_EINVAL, "%s: null options", who);
  if (O->length_min < 1) return fail(VSX_EINVAL, "%s: length_min must be at least 1", who);
  if (O->parents_max < 2 || O->parents_max > VSX_CHIMERAS_LONG_MAX_PARENTS) return fail(VSX_EINVAL, "%s: parents_max must be in the range 2 to 20", who);
  if (!(O->diff_pct >= 0.0 && O->diff_pct <= 50.0)) return fail(VSX_EINVAL, "%s: diff_pct must be in the range 0.0 to 50.0", who);
  if (O->parts != 0 && (O->parts < 2 || O->parts > 100)) return fail(VSX_EINVAL, "%s: parts must be 0 (by length) or in the range 2 to 100", who);
  if (!(O->abskew >= 1.0)) return fail(VSX_EINVAL, "%s: abskew must be >= 1.0", who);
  return VSX_OK;
}

int vsx_chimeras_denovo(vsx_searcher * S, const vsx_chimeras_long_opts * O, vsx_chimeras_long_result * out)
{
  g_lstats = vsx_chimera_denovo_stats {};
  const double t0 = now_s();
  int rc = chimeras_long_check(O, "vsx_chimeras_denovo");
  if (rc != VSX_OK) return rc;
  if (!S || !out) return fail(VSX_EINVAL, "vsx_chimeras_denovo: null argument");
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);
  if (so.strand_both) return fail(VSX_EINVAL, "vsx_chimeras_denovo: --strand both is not provided (the reference refuses it)");
  if (so.id != 0.55 || so.weak_id != 0.55 || so.maxaccepts != 4 || so.maxrejects != 16 || so.cluster_unoise || so.self != 1 ||
      so.selfid != 1 || so.maxsizeratio != 1.0 / O->abskew || (so.qmask != 0 && so.qmask != so.soft_mask + 1))
    return fail(VSX_EINVAL, "vsx_chimeras_denovo: the searcher was not created with the detection parameters (vsx_chimeras_long_opts_default: "
                             "id = weak_id = 0.55, maxaccepts 4, maxrejects 16, self = selfid = 1, maxsizeratio = 1 / abskew, qmask as soft_mask)");
  if (!vsx_internal_searcher_has_abundances(S)) return fail(VSX_EINVAL, "vsx_chimeras_denovo: the searcher has no abundances (vsx_searcher_set_meta)");
  if (so.wordlength > 8) return fail(VSX_EINVAL, "vsx_chimeras_denovo: word lengths above 8 are not provided");
  const uint64_t n = vsx_seqset_count(vsx_internal_searcher_dbset(S));
  if (n == 0) { g_lstats.seconds_total = now_s() - t0; return VSX_OK; }
  VsxDenovo * D = nullptr;
  rc = vsx_internal_denovo_create(S, &D);
  if (rc != VSX_OK) return rc;
  struct DGuard { VsxDenovo * d; ~DGuard() { vsx_internal_denovo_destroy(d); } } dg {D};
  const bool host_all = vsxp::env_is_host("VSX_CHIMERA");
  const uint64_t window = O->window > 0 ? (uint64_t) O->window : 4096;
  CallBufs bufs;
  LongMode mode {VsxChimLongParams {O->parents_max, O->length_min, O->diff_pct, 0, 0}, O->parts, (uint32_t) so.maxaccepts, bufs, host_all};
  std::vector<uint32_t> commit;
  for (uint64_t s0 = 0; s0 < n; s0 += window)
    {
      commit.clear();
      rc = denovo_window(S, D, mode, g_lstats, s0, std::min(window, n - s0), out, commit);
      if (rc != VSX_OK) return rc;
      vsx_internal_denovo_commit(D, commit);
      ++g_lstats.windows;
    }
  g_lstats.seconds_total = now_s() - t0;
  return VSX_OK;
}

int vsx_internal_chimeras_long_host(const char * q, uint32_t qlen, uint32_t nc, const char * const * t, const uint32_t * tlen,
                                    const char * const * cigars, const vsx_chimeras_long_opts * O, vsx_chimeras_long_result * out)
{
  int rc = chimeras_long_check(O, "vsx_internal_chimeras_long_host");
  if (rc != VSX_OK) return rc;
  if (!out || (qlen && !q) || (nc && (!t || !tlen || !cigars))) return fail(VSX_EINVAL, "vsx_internal_chimeras_long_host: null argument");
  std::vector<uint8_t> qcode(qlen);
  for (uint32_t i = 0; i < qlen; ++i) qcode[i] = map4((unsigned char) q[i]);
  std::vector<std::vector<uint8_t>> tcode(nc);
  std::vector<std::vector<uint32_t>> runs(nc);
  std::vector<const uint8_t *> tp(nc);
  std::vector<uint32_t> cand(nc);
  for (uint32_t c = 0; c < nc; ++c)
    {
      tcode[c].resize(tlen[c]);
      for (uint32_t i = 0; i < tlen[c]; ++i) tcode[c][i] = map4((unsigned char) t[c][i]);
      tp[c] = tcode[c].data();
      cand[c] = c;
      runs[c] = runs_from_text(cigars[c]);
      uint64_t qn = 0, tn = 0;
      for (uint32_t w : runs[c]) { if ((w & 3u) != 1u) qn += w >> 2; if ((w & 3u) != 2u) tn += w >> 2; }
      if (qn != qlen || tn != tlen[c]) return fail(VSX_EINVAL, "vsx_internal_chimeras_long_host: CIGAR %u does not span the two sequences", c);
    }
  vsx_internal_chimeras_long_eval_host(qcode.data(), (int) qlen, (int) nc, cand.data(), runs, tp,
                                       VsxChimLongParams {O->parents_max, O->length_min, O->diff_pct, 0, 0}, out);
  return VSX_OK;
}

}  // extern "C"
