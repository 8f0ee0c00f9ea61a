// vsx_chimera.cpp -- --uchime_ref dispatch (include/vsx_search.h vsx_uchime_ref) and the host restatement of its selection and scoring.
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

#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

extern "C" void vsx_internal_set_error(const char * msg);
extern "C" int vsx_internal_device(const vsx_ctx * ctx);
extern "C" hipStream_t vsx_internal_stream(const vsx_ctx * ctx);
extern "C" void vsx_internal_seqset_device(const vsx_seqset * s, const uint8_t ** codes, const uint64_t ** off, const uint32_t ** len, uint64_t * n);
extern "C" vsx_ctx * vsx_internal_searcher_ctx(const vsx_searcher * S);
extern "C" const vsx_search_opts * vsx_internal_searcher_opts(const vsx_searcher * S);
extern "C" const vsx_scoring * vsx_internal_searcher_scoring(const vsx_searcher * S);
extern "C" const vsx_seqset * vsx_internal_searcher_dbset(const vsx_searcher * S);
extern "C" int vsx_internal_search_parts(vsx_searcher * S, int64_t tophits, uint64_t nq, const char * qblob, uint64_t qbytes,
                                         const uint64_t * qoff, const uint32_t * qlen, vsx_hits * out);
extern "C" void vsx_internal_searcher_text(const vsx_searcher * S, const char ** blob, const uint64_t ** off, const uint32_t ** len);

namespace {

thread_local vsx_chimera_stats g_stats {};

constexpr int kParts = 4;            // chimera_info->parts for uchime (:302-304)
constexpr int kWindow = 32;          // `window` (:110)
constexpr uint32_t kNone = 0xFFFFFFFFu;

int cfail(int code, const std::string & msg) { vsx_internal_set_error(msg.c_str()); return code; }

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// chrmap_4bit (utils/maps.cpp): the codes the device encoder writes into a sequence set
uint8_t map4(unsigned char c)
{
  switch (c | 0x20)
    {
    case 'a': return 1;  case 'b': return 14; case 'c': return 2;  case 'd': return 13;
    case 'g': return 4;  case 'h': return 11; case 'k': return 12; case 'm': return 3;
    case 'n': return 15; case 'r': return 5;  case 's': return 6;  case 't': return 8;
    case 'u': return 8;  case 'v': return 7;  case 'w': return 9;  case 'y': return 10;
    default: return 0;
    }
}

bool ambiguous4(uint8_t c) { return c != 1 && c != 2 && c != 4 && c != 8; }     // chrmap_ambiguous_4bit

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
  if (best_h >= P.minh)
    {
      r->flag = '?';
      if ((divdiff >= P.mindiv) && (sumL >= P.mindiffs) && (sumR >= P.mindiffs)) r->flag = 'Y';
    }
}

namespace {

// device buffers of one vsx_uchime_ref call, grown as windows need them (a hipFree synchronises the whole device)
template <class T>
struct GrowBuf {
  T * p = nullptr;
  size_t cap = 0;
  ~GrowBuf() { if (p) (void) hipFree(p); }
  hipError_t reserve(size_t n)
  {
    if (n <= cap) return hipSuccess;
    if (p) { const hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    n = std::max<size_t>(n, cap * 3 / 2 + 1);
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
};
struct CallBufs {
  GrowBuf<VsxPairOut> hits;
  GrowBuf<uint32_t> runs;
  GrowBuf<VsxChimItem> items;
  GrowBuf<vsx_chimera_result> out;
};

#define CHIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return cfail(VSX_EHIP, std::string("vsx_uchime_ref: ") + hipGetErrorString(e_)); } while (0)

// one window: queries [w0, w0 + nw) of the call
int run_window(vsx_searcher * S, const vsx_chimera_opts & O, CallBufs & B, bool host_all, uint64_t w0, uint64_t nw, const char * qblob, uint64_t qbytes,
               const uint64_t * qoff, const uint32_t * qlen, vsx_chimera_result * out)
{
  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  const char * dbtext;
  const uint64_t * dboff;
  const uint32_t * dblen;
  vsx_internal_searcher_text(S, &dbtext, &dboff, &dblen);
  const VsxChimParams P {O.minh, O.mindiv, O.xn, O.dn, O.mindiffs};
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);

  // 1-2. parts through the window search
  double t0 = now_s();
  std::vector<uint64_t> poff;
  std::vector<uint32_t> plen, pquery;
  for (uint64_t k = 0; k < nw; ++k)
    {
      const uint32_t L = qlen[w0 + k];
      if (L < (uint32_t) kParts) continue;
      uint32_t rest = L;
      uint64_t cur = qoff[w0 + k];
      for (int i = 0; i < kParts; ++i)
        {
          const uint32_t length = (rest + (uint32_t) (kParts - i - 1)) / (uint32_t) (kParts - i);
          poff.push_back(cur);
          plen.push_back(length);
          pquery.push_back((uint32_t) k);
          rest -= length;
          cur += length;
        }
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
  const double t1 = now_s();
  g_stats.seconds_search += t1 - t0;

  // 4. whole queries against their candidates: one plan for the window
  std::vector<uint32_t> qidx, tidx, pair0(nw, 0);
  std::vector<uint64_t> woff(nw);
  std::string wblob;
  for (uint64_t k = 0; k < nw; ++k)
    {
      woff[k] = wblob.size();
      wblob.append(qblob + qoff[w0 + k], qlen[w0 + k]);
      if (ncand[k] < 2 || qlen[w0 + k] < (uint32_t) kWindow) continue;        // no two parents possible
      pair0[k] = (uint32_t) qidx.size();
      for (uint32_t c = 0; c < ncand[k]; ++c) { qidx.push_back((uint32_t) k); tidx.push_back(cand[(size_t) k * VSX_CHIM_MAXCAND + c]); }
    }
  for (uint64_t k = 0; k < nw; ++k)
    if (ncand[k] < 2 || qlen[w0 + k] < (uint32_t) kWindow) unscored(&out[w0 + k], VSX_CHIMERA_NO_PARENTS, kNone, kNone);
  if (qidx.empty()) return VSX_OK;

  vsx_seqset * qs = nullptr;
  int rc = vsx_seqset_create(ctx, &qs, nw, wblob.data(), wblob.size(), woff.data(), qlen + w0);
  if (rc != VSX_OK) return rc;
  struct Guard { vsx_seqset * s; vsx_plan * p = nullptr; ~Guard() { vsx_plan_destroy(p); vsx_seqset_destroy(s); } } g {qs};
  rc = vsx_plan_create(ctx, &g.p, qs, dbset, qidx.size(), qidx.data(), tidx.data(), 0);
  if (rc == VSX_OK) rc = vsx_plan_run(g.p);
  if (rc == VSX_OK) rc = vsx_plan_sync(g.p, nullptr);
  if (rc != VSX_OK) return rc;
  const uint64_t npairs = qidx.size();
  CHIP(hipSetDevice(vsx_internal_device(ctx)));
  GrowBuf<VsxPairOut> & d_hits = B.hits;
  CHIP(d_hits.reserve(npairs));
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
  GrowBuf<uint32_t> & d_runs = B.runs;
  CHIP(d_runs.reserve(std::max<uint64_t>(nruns, 1)));
  if (nruns) { rc = vsx_plan_export_runs(g.p, d_runs.p, nruns * 4, &nruns); if (rc != VSX_OK) return rc; }
  std::vector<VsxPairOut> h_hits(npairs);
  CHIP(hipMemcpy(h_hits.data(), d_hits.p, npairs * sizeof(VsxPairOut), hipMemcpyDeviceToHost));
  const double t2 = now_s();
  g_stats.seconds_align += t2 - t1;
  g_stats.pairs_aligned += npairs;

  // every run list the evaluation reads must lie inside the exported buffer: checked here for both routes, so that a bad export
  // fails the call the same way whichever route a query takes (the kernel's own bound check only keeps it inside the buffer)
  for (uint64_t p = 0; p < npairs; ++p)
    if (h_hits[p].score != VSX_SCORE_SENTINEL && h_hits[p].run_off + h_hits[p].nruns > nruns)
      return cfail(VSX_EHIP, "vsx_uchime_ref: run words out of range");

  // 5. route: kernel, or host restatement (long query, sentinel pair, VSX_CHIMERA=host)
  std::vector<VsxChimItem> items;
  std::vector<uint64_t> host_q;
  for (uint64_t k = 0; k < nw; ++k)
    {
      if (ncand[k] < 2 || qlen[w0 + k] < (uint32_t) kWindow) continue;
      bool sentinel = false;
      for (uint32_t c = 0; c < ncand[k]; ++c)
        if (h_hits[pair0[k] + c].score == VSX_SCORE_SENTINEL) { sentinel = true; ++g_stats.sentinel_pairs; }
      if (host_all || sentinel || qlen[w0 + k] > VSX_CHIMERA_MAX_QLEN) { host_q.push_back(k); continue; }
      VsxChimItem it {};
      it.q = (uint32_t) k;
      it.ncand = ncand[k];
      it.pair0 = pair0[k];
      it.out = (uint32_t) items.size();
      std::copy(&cand[(size_t) k * VSX_CHIM_MAXCAND], &cand[(size_t) k * VSX_CHIM_MAXCAND] + VSX_CHIM_MAXCAND, it.cand);
      items.push_back(it);
    }
  if (!items.empty())
    {
      const uint8_t * qc, * tc;
      const uint64_t * qo, * to;
      const uint32_t * ql, * tl;
      uint64_t dummy;
      vsx_internal_seqset_device(qs, &qc, &qo, &ql, &dummy);
      vsx_internal_seqset_device(dbset, &tc, &to, &tl, &dummy);
      hipStream_t st = vsx_internal_stream(ctx);
      GrowBuf<VsxChimItem> & d_items = B.items;
      GrowBuf<vsx_chimera_result> & d_out = B.out;
      CHIP(d_items.reserve(items.size()));
      CHIP(d_out.reserve(items.size()));
      CHIP(hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(VsxChimItem), hipMemcpyHostToDevice, st));
      CHIP(vsx_launch_chimera_eval(d_items.p, (uint32_t) items.size(), qc, qo, ql, tc, to, tl, d_hits.p, d_runs.p, nruns, P, d_out.p, st));
      std::vector<vsx_chimera_result> res(items.size());
      CHIP(hipMemcpyAsync(res.data(), d_out.p, res.size() * sizeof(vsx_chimera_result), hipMemcpyDeviceToHost, st));
      CHIP(hipStreamSynchronize(st));
      for (const VsxChimItem & it : items) out[w0 + it.q] = res[it.out];
      g_stats.queries_kernel += items.size();
    }
  if (!host_q.empty())
    {
      std::vector<uint32_t> h_runs(nruns);
      if (nruns) CHIP(hipMemcpy(h_runs.data(), d_runs.p, nruns * 4, hipMemcpyDeviceToHost));
      const vsx_scoring * sc = vsx_internal_searcher_scoring(S);
      std::vector<uint8_t> qcode;
      std::vector<std::vector<uint8_t>> tcode;
      for (uint64_t k : host_q)
        {
          const uint32_t L = qlen[w0 + k];
          const char * qt = qblob + qoff[w0 + k];
          qcode.resize(L);
          for (uint32_t i = 0; i < L; ++i) qcode[i] = map4((unsigned char) qt[i]);
          const uint32_t nc = ncand[k];
          const uint32_t * ck = &cand[(size_t) k * VSX_CHIM_MAXCAND];
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
          vsx_internal_chimera_eval_host(qcode.data(), (int) L, (int) nc, ck, runs, tp, P, &out[w0 + k]);
        }
      g_stats.queries_host += host_q.size();
    }
  g_stats.seconds_eval += now_s() - t2;
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
  if (!S || !O || (n && (!qblob || !qoff || !qlen || !out))) return cfail(VSX_EINVAL, "vsx_uchime_ref: null argument");
  const vsx_search_opts & so = *vsx_internal_searcher_opts(S);
  if (so.id != 0.55 || so.weak_id != 0.55 || so.maxaccepts != 4 || so.maxrejects != 16 || so.strand_both || so.cluster_unoise || so.self)
    return cfail(VSX_EINVAL, "vsx_uchime_ref: the searcher was not created with the detection parameters (vsx_chimera_opts_default: "
                             "id = weak_id = 0.55, maxaccepts 4, maxrejects 16, plus strand)");
  if (O->mindiffs < 0 || !(O->xn > 0.0) || !(O->dn >= 0.0)) return cfail(VSX_EINVAL, "vsx_uchime_ref: xn must be > 0, dn >= 0, mindiffs >= 0");
  for (uint64_t k = 0; k < n; ++k)
    if (qoff[k] + qlen[k] > qbytes) return cfail(VSX_EINVAL, "vsx_uchime_ref: query exceeds the blob");
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

}  // extern "C"
