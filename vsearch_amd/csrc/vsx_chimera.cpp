// vsx_chimera.cpp -- --uchime_ref and de novo chimera dispatch (include/vsx_search.h vsx_uchime_ref, vsx_uchime_denovo) and the host
// restatement of the selection and scoring.  The de novo loop (denovo_window below) reuses steps 4-5; its part search lives in
// vsx_denovo_search.cpp (vsx_internal_denovo_*).
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

// device buffers of one call, replaced when a window needs more (a hipFree synchronises the whole device)
struct CallBufs {
  DevBuf<VsxPairOut> hits;
  DevBuf<uint32_t> runs;
  DevBuf<VsxChimItem> items;
  DevBuf<vsx_chimera_result> out;
};

// one query of steps 4-5: its index in the query set of the plan, its text, its candidate parents and where its record goes
struct EvalJob {
  uint32_t q;
  const char * text;
  uint32_t len;
  uint32_t ncand;
  const uint32_t * cand;
  vsx_chimera_result * out;
};
struct EvalAcct { double t_align = 0, t_eval = 0; uint64_t pairs = 0, sentinels = 0, kernel = 0, host = 0; };

// 4. whole queries against their candidates: one plan of (job.q in qset, candidate in the database set) pairs; 5. selection + scoring
// on the kernel, or on the host restatement (long query, sentinel pair, host_all).  A job with < 2 candidates, or shorter than the
// 32-column window, cannot get two parents and is answered at once.
int align_and_eval(vsx_searcher * S, const VsxChimParams & P, CallBufs & B, bool host_all, const vsx_seqset * qset,
                   const std::vector<EvalJob> & jobs, EvalAcct & A, const char * who)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  const char * dbtext;
  const uint64_t * dboff;
  const uint32_t * dblen;
  vsx_internal_searcher_text(S, &dbtext, &dboff, &dblen);
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

  struct Guard { vsx_plan * p = nullptr; ~Guard() { vsx_plan_destroy(p); } } g;
  int rc = vsx_plan_create(ctx, &g.p, qset, dbset, qidx.size(), qidx.data(), tidx.data(), 0);
  if (rc == VSX_OK) rc = vsx_plan_run(g.p);
  if (rc == VSX_OK) rc = vsx_plan_sync(g.p, nullptr);
  if (rc != VSX_OK) return rc;
  const uint64_t npairs = qidx.size();
  VSX_HIP_AS(who, hipSetDevice(vsx_internal_device(ctx)));
  DevBuf<VsxPairOut> & d_hits = B.hits;
  VSX_HIP_AS(who, d_hits.ensure(npairs));
  rc = vsx_plan_export_hits(g.p, d_hits.p, npairs * sizeof(VsxPairOut));
  if (rc != VSX_OK) return rc;
  uint64_t nruns = 0;
  if (vsx_plan_export_runs(g.p, nullptr, 0, &nruns) != VSX_OK)
    {
      // the run buffer overflowed: vsx_plan_fetch resizes it and runs the traceback again
      vsx_results tmp {};
      rc = vsx_plan_fetch(g.p, &tmp);
      vsx_results_free(&tmp);
      if (rc != VSX_OK) return rc;
      rc = vsx_plan_export_hits(g.p, d_hits.p, npairs * sizeof(VsxPairOut));
      if (rc == VSX_OK) rc = vsx_plan_export_runs(g.p, nullptr, 0, &nruns);
      if (rc != VSX_OK) return rc;
    }
  DevBuf<uint32_t> & d_runs = B.runs;
  VSX_HIP_AS(who, d_runs.ensure(std::max<uint64_t>(nruns, 1)));
  if (nruns) { rc = vsx_plan_export_runs(g.p, d_runs.p, nruns * 4, &nruns); if (rc != VSX_OK) return rc; }
  std::vector<VsxPairOut> h_hits(npairs);
  VSX_HIP_AS(who, hipMemcpy(h_hits.data(), d_hits.p, npairs * sizeof(VsxPairOut), hipMemcpyDeviceToHost));
  const double t2 = now_s();
  A.t_align += t2 - t1;
  A.pairs += npairs;

  // every run list the evaluation reads must lie inside the exported buffer: checked here for both routes, so that a bad export
  // fails the call the same way whichever route a query takes (the kernel's own bound check only keeps it inside the buffer)
  for (uint64_t p = 0; p < npairs; ++p)
    if (h_hits[p].score != VSX_SCORE_SENTINEL && h_hits[p].run_off + h_hits[p].nruns > nruns)
      return fail(VSX_EHIP, "%s: run words out of range", who);

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
      const vsx_scoring * sc = vsx_internal_searcher_scoring(S);
      std::vector<uint8_t> qcode;
      std::vector<std::vector<uint8_t>> tcode;
      for (size_t k : host_q)
        {
          const EvalJob & j = jobs[k];
          const uint32_t L = j.len;
          const char * qt = j.text;
          qcode.resize(L);
          for (uint32_t i = 0; i < L; ++i) qcode[i] = map4((unsigned char) qt[i]);
          const uint32_t nc = j.ncand;
          const uint32_t * ck = j.cand;
          std::vector<std::vector<uint32_t>> runs(nc);
          std::vector<const uint8_t *> tp(nc);
          tcode.assign(nc, {});
          for (uint32_t c = 0; c < nc; ++c)
            {
              const char * tt = dbtext + dboff[ck[c]];
              const uint32_t tl = dblen[ck[c]];
              tcode[c].resize(tl);
              for (uint32_t i = 0; i < tl; ++i) tcode[c][i] = map4((unsigned char) tt[i]);
              tp[c] = tcode[c].data();
              const VsxPairOut & h = h_hits[pair0[k] + c];
              if (h.score == VSX_SCORE_SENTINEL)
                {
                  int64_t score, alen, ma, mi, ga;
                  char * cig = nullptr;
                  rc = vsx_lma_align(sc, qt, L, tt, tl, &score, &alen, &ma, &mi, &ga, &cig);
                  if (rc != VSX_OK) return rc;
                  runs[c] = runs_from_text(cig);
                  std::free(cig);
                }
              else
                {
                  runs[c].assign(h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off - h.nruns), h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off));
                }
            }
          vsx_internal_chimera_eval_host(qcode.data(), (int) L, (int) nc, ck, runs, tp, P, j.out);
        }
      A.host += host_q.size();
    }
  A.t_eval += now_s() - t2;
  return VSX_OK;
}

// the 4 parts of a query of length L >= 4 (partition_query, :1930-1955): lengths of the integer split, front to back
template <class F>
void for_each_part(uint32_t L, F && f)
{
  uint32_t rest = L, at = 0;
  for (int i = 0; i < kParts; ++i)
    {
      const uint32_t length = (rest + (uint32_t) (kParts - i - 1)) / (uint32_t) (kParts - i);
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
      for_each_part(L, [&](uint32_t at, uint32_t length) { poff.push_back(qoff[w0 + k] + at); plen.push_back(length); pquery.push_back((uint32_t) k); });
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

thread_local vsx_chimera_denovo_stats g_dstats {};

// status < suspicious (chimera.cpp:2314, :2365): what joins the index of later queries
bool nonchimeric(const vsx_chimera_result & r) { return r.flag == 'N'; }

// One window [s0, s0 + wn) of vsx_uchime_denovo: speculative passes with an in-order fix-up.
//   present[j]  member j's assumed status in the current pass: its final one when resolved, "non-chimera" while pending
//   lists[p]    part p's merged candidate list of the pass that produced the query's current result
//   deps[k]     the earlier members that appeared in one of query k's lists
// A pass re-searches, re-aligns and re-evaluates only the pending queries whose lists changed; a pending query whose lists did not
// change keeps its result (the same lists give the same search, the same parents and the same scores).  A member reaches a list only
// while it is assumed present, so query k is final once every member in deps[k] is final and a non-chimera: a member that did not
// reach a list could only have pushed others out, and a pending member assumed present that turns out chimeric leaves the lists it
// was not in unchanged.  The first pending query sees only final members, so every pass resolves at least one query.
int denovo_window(vsx_searcher * S, VsxDenovo * D, const vsx_chimera_denovo_opts & O, CallBufs & B, bool host_all, uint64_t s0, uint64_t wn,
                  vsx_chimera_result * out, std::vector<uint32_t> & commit)
{
  const char * text;
  const uint64_t * off;
  const uint32_t * len;
  vsx_internal_searcher_text(S, &text, &off, &len);
  const VsxChimParams P {O.base.minh, O.base.mindiv, O.base.xn, O.base.dn, O.base.mindiffs, O.variant};

  std::vector<uint64_t> poff;
  std::vector<uint32_t> plen, pmember, part0(wn + 1, 0);
  for (uint64_t k = 0; k < wn; ++k)
    {
      part0[k] = (uint32_t) poff.size();
      const uint32_t L = len[s0 + k];
      if (L >= (uint32_t) kParts)
        for_each_part(L, [&](uint32_t at, uint32_t length) { poff.push_back(off[s0 + k] + at); plen.push_back(length); pmember.push_back((uint32_t) k); });
    }
  part0[wn] = (uint32_t) poff.size();
  g_dstats.parts += poff.size();
  int rc = vsx_internal_denovo_window(D, s0, wn, poff, plen, pmember, &g_dstats.seconds_rank, &g_dstats.seconds_members);
  if (rc != VSX_OK) return rc;

  std::vector<uint8_t> present(wn, 1), final_(wn, 0), done_once(wn, 0);
  std::vector<std::vector<uint32_t>> lists(poff.size()), deps(wn);
  std::vector<uint32_t> ncand(wn, 0), cand(wn * VSX_CHIM_MAXCAND, 0);
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
          if (done_once[k]) ++g_dstats.queries_reevaluated;
          done_once[k] = 1;
          redo.push_back(k);
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p) parts.push_back(p);
          deps[k].clear();
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p)
            for (uint32_t t : lists[p])
              if (t >= s0 && std::find(deps[k].begin(), deps[k].end(), (uint32_t) (t - s0)) == deps[k].end()) deps[k].push_back((uint32_t) (t - s0));
        }
      g_dstats.seconds_reconcile += now_s() - t0;

      // the parts of those queries through the staged search; accepted hits part by part, repeated targets dropped (:2017-2071)
      t0 = now_s();
      std::vector<std::vector<uint32_t>> acc;
      rc = vsx_internal_denovo_search(D, parts, acc, &g_dstats.pairs_searched, &g_dstats.sentinel_pairs);
      if (rc != VSX_OK) return rc;
      g_dstats.seconds_search += now_s() - t0;
      size_t x = 0;
      for (uint32_t k : redo)
        {
          ncand[k] = 0;
          uint32_t * c = &cand[(size_t) k * VSX_CHIM_MAXCAND];
          for (uint32_t p = part0[k]; p < part0[k + 1]; ++p, ++x)
            for (uint32_t tg : acc[x])
              if (std::find(c, c + ncand[k], tg) == c + ncand[k] && ncand[k] < VSX_CHIM_MAXCAND) c[ncand[k]++] = tg;
        }

      // whole queries (in the database set) against their candidates, selection + scoring
      if (!redo.empty())
        {
          std::vector<EvalJob> jobs;
          jobs.reserve(redo.size());
          for (uint32_t k : redo)
            jobs.push_back(EvalJob {(uint32_t) (s0 + k), text + off[s0 + k], len[s0 + k], ncand[k], &cand[(size_t) k * VSX_CHIM_MAXCAND], &out[s0 + k]});
          EvalAcct A;
          rc = align_and_eval(S, P, B, host_all, vsx_internal_searcher_dbset(S), jobs, A, "vsx_uchime_denovo");
          if (rc != VSX_OK) return rc;
          g_dstats.seconds_align += A.t_align;
          g_dstats.seconds_eval += A.t_eval;
          g_dstats.pairs_aligned += A.pairs;
          g_dstats.sentinel_pairs += A.sentinels;
          g_dstats.queries_kernel += A.kernel;
          g_dstats.queries_host += A.host;
        }

      // validate in order
      t0 = now_s();
      std::vector<uint32_t> still;
      for (uint32_t k : pending)
        {
          bool ok = true;
          for (uint32_t j : deps[k])
            if (!final_[j] || !nonchimeric(out[s0 + j])) { ok = false; break; }          // (a member in a list was assumed present)
          if (ok) { final_[k] = 1; present[k] = nonchimeric(out[s0 + k]) ? 1 : 0; }
          else still.push_back(k);
        }
      pending.swap(still);
      g_dstats.seconds_reconcile += now_s() - t0;
    }
  g_dstats.passes += passes;
  g_dstats.passes_max = std::max<uint64_t>(g_dstats.passes_max, passes);
  for (uint64_t k = 0; k < wn; ++k)
    if (present[k]) commit.push_back((uint32_t) (s0 + k));
  return VSX_OK;
}

}  // namespace

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
  for (uint64_t k = 0; k < n; ++k)
    if (qoff[k] + qlen[k] > qbytes) return fail(VSX_EINVAL, "vsx_uchime_ref: query exceeds the blob");
  const char * env = std::getenv("VSX_CHIMERA");
  const bool host_all = env && std::strcmp(env, "host") == 0;
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
  const char * env = std::getenv("VSX_CHIMERA");
  const bool host_all = env && std::strcmp(env, "host") == 0;
  const uint64_t window = O->base.window > 0 ? (uint64_t) O->base.window : 4096;
  CallBufs bufs;
  std::vector<uint32_t> commit;
  for (uint64_t s0 = 0; s0 < n; s0 += window)
    {
      commit.clear();
      rc = denovo_window(S, D, *O, bufs, host_all, s0, std::min(window, n - s0), out, commit);
      if (rc != VSX_OK) return rc;
      vsx_internal_denovo_commit(D, commit);
      ++g_dstats.windows;
    }
  g_dstats.seconds_total = now_s() - t0;
  return VSX_OK;
}

}  // extern "C"
